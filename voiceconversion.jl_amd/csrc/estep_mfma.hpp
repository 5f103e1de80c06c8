// estep_mfma.hpp -- estep_mfma_kernel, the FP64 MFMA kernel of the diagonal E-step (included by estep.hip; M <= 128 per launch,
// even Dj <= 160).  EstepCfg<DJ> -- tiles, LDS layout, the one-kernel / two-kernel (SPLIT) forms: estep_cfg.hpp.
#pragma once
#include "estep_cfg.hpp"

namespace vcmi {

// Wpack: [mt (8)][ks (KS)][lane (64)] A-operand fragments of W = [-iv/2 | mu*iv] (rows = mixtures), zero rows for m >= M
// cinit: [128] log-density constants c_m (-inf rows for m >= M so that their gamma is exactly 0)
// PHASE 0: the whole E-step in one kernel.  PHASE 1 / 2 (EstepCfg::SPLIT): responsibilities -> G (frames x 128, row-major)
// and the log-likelihood / statistics from G.  PHASE 3 (more than 128 mixtures: one launch per GROUP of 128): as PHASE 1,
// normalised within the group, plus the group's log-sum-exp of every frame written to `part[frame]`; the groups are
// combined by estep_group_combine_kernel and the statistics taken per group by PHASE 2.
template <int DJ, int PHASE, bool SHARE>
__global__ void __launch_bounds__(512)
estep_mfma_kernel(const double *__restrict__ X, int64_t N, int M, const double *__restrict__ Wpack,
                  const double *__restrict__ cinit, double *__restrict__ part, int64_t plen,
                  const double *__restrict__ refmu, const double *__restrict__ refiv, const double *__restrict__ refc,
                  double *__restrict__ G, int dj, int mtp_arg, unsigned long long *__restrict__ mfma_count,
                  const int64_t *__restrict__ Ndev) {
  if (Ndev) {                                // (the soft frames of estep_hard.hpp: their number exists on the device only)
    N = *Ndev;
    if (N == 0) return;                      // none: no partials either -- estep_reduce_kernel is told the same way and leaves the statistics alone
  }
  // mfma_count (optional, measurement): v_mfma_f64_16x16x4 instructions issued, counted by wave-uniform scalar adds
  // mtp = 1, 2, 4 or 8 mixture tiles of 16 (>= M / 16): with fewer than eight (SHARE), 8 / mtp waves share a tile -- wave
  // w takes tile w % mtp and every (8 / mtp)-th frame tile of step A / k-step of step B, and writes its own row of
  // partial statistics -- so that a 16- or 64-mixture model does not pay for 128 slots.  (A template flag: the branches
  // cost the full-width kernel 3.5 % when they are run-time decisions.)
  const int mtp = SHARE ? mtp_arg : 8;
  // dj <= DJ is the data's joint dimension (even: rows of X are 16-byte aligned), DJ the instantiated one: the columns
  // dj .. DJ-1 of the LDS image hold other (finite) values of X, meet zero weights in step A and statistics in step B
  // that are never written out
  using C = EstepCfg<DJ>;
  constexpr int KS = C::KS, NDT = C::NDT, FB = C::FB, RSX = C::RSX, RSG = C::RSG, XBUF = C::XBUF;
  constexpr bool kGamma = PHASE != 2, kStats = (PHASE == 0 || PHASE == 2);
  constexpr int kStepBUnroll = PHASE == 0 ? 4 : FB / 4;
  extern __shared__ double smem[];
  double *xbuf = smem;                     // [2][XBUF]: [FB][RSX] images
  double *lg = smem + 2 * XBUF;            // [FB][RSG]   l, then gamma
  double *red = lg;                        // [8][64] scratch for the log-likelihood reduction (epilogue only)
  double *etab = lg + FB * RSG;            // [64] 2^(j/64) for vc_exp_tab (fp64_exp.hpp)
  // PHASE 0: step B takes the block's frames GROUPED BY THE MIXTURE TILE THAT WINS THEM.  Its k-steps are 4 frames x the wave's
  // 16 mixtures and are skipped when all 64 responsibilities are exactly zero; in the order the frames arrive, a tile's
  // few frames are spread over most k-steps (BASELINE data: 41 % of the k-steps survive), grouped they sit in two or three.
  // A sum over frames does not depend on their order (rounding aside: the statistics stay deterministic, run to run).
  // (fkey / fperm / kSortB: below, after the lane indices)
  if (threadIdx.x < 64) etab[threadIdx.x] = kExp2Tab[threadIdx.x];       // (visible after the barrier behind the first stage)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lcol = lane & 15, lgrp = lane >> 4;
  double *tthr = etab + 64;                         // [MMAX] refinement thresholds (refc[2 m + 1]; -inf: the expanded form is always good enough)
  if (kGamma && threadIdx.x < C::MMAX) tthr[threadIdx.x] = ((int)threadIdx.x < M) ? refc[2 * threadIdx.x + 1] : -INFINITY;
  int *fkey = reinterpret_cast<int *>(tthr + C::MMAX);   // [FB] winning tile of each frame (softmax phase)
  int *fperm = fkey + FB + wave * FB;               // [FB] this wave's copy of the grouped order
  constexpr bool kSortB = (PHASE == 0);
  const int tile = SHARE ? (wave & (mtp - 1)) : wave, sub = SHARE ? wave / mtp : 0, wpt = SHARE ? 8 / mtp : 1;      // mixture tile, position among the tile's waves

  // this wave's weight fragments and log-density constants stay in registers for the whole kernel
  double wfrag[kGamma ? KS : 1];
  if constexpr (kGamma) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wfrag[ks] = Wpack[((size_t)tile * KS + ks) * 64 + lane];
  }
  // step A computes the TRANSPOSED tile (rows = frames, cols = this wave's mixtures) by swapping the MFMA operands:
  // the result then lands in LDS with lanes along consecutive mixtures -> conflict-free stores
  const double cm = kGamma ? cinit[16 * tile + lcol] : 0.0;
  const d4 cin = {cm, cm, cm, cm};

  d4 sacc[kStats ? NDT : 1];   // statistics tiles: rows = this wave's 16 mixtures, cols = 16 of the 2*DJ columns [x | x^2]
  double s0l = 0.0;   // sum over this lane's frames of gamma[f][m = 16 wave + lcol]
#pragma unroll
  for (int j = 0; j < (kStats ? NDT : 1); ++j) sacc[j] = d4{0, 0, 0, 0};
  double llacc = 0.0, sprod = 1.0;
  int nprod = 0;
  int nmfma = 0;

  const int64_t nblocks = (N + FB - 1) / FB;
  // ---- x staging by LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane straight into LDS, no VGPRs -- the kernel has
  //      none to spare): a wave-instruction fills 1 KB of the padded [FB][RSX] image; lanes that fall into a row's
  //      16-byte pad, and frames beyond N, fetch a valid address (frame N-1 / the block start) and are never used ----
  constexpr int ROWB = RSX * 8, NCHUNK = XBUF / 128;      // (the last wave-instruction may run into the buffer's padding)
  auto stage = [&](int64_t f0, double *dst) {
    const char *base = reinterpret_cast<const char *>(X + f0 * dj);          // workgroup-uniform 64-bit base,
    const int last = (int)((N - 1 - f0 < FB - 1) ? N - 1 - f0 : FB - 1);     // 32-bit per-lane offsets
    // The per-lane (row, column) of every chunk is loop-invariant; hoisted out of the block loop it costs 9 VGPRs this
    // kernel does not have -- they were spilled and came back from scratch behind four exposed s_waitcnt vmcnt per
    // block.  The opaque copy of the lane id makes them a handful of integer instructions per block instead.
    int lane_v = lane;
    asm volatile("" : "+v"(lane_v));
#pragma unroll
    for (int i = 0; i < (NCHUNK + 7) / 8; ++i) {
      const int q = wave + 8 * i;
      if (q < NCHUNK) {                                          // wave-uniform
        const int o = 1024 * q + 16 * lane_v, row = o / ROWB, col = o - row * ROWB;
        const int rowc = row < last ? row : last;      // (also rows >= FB of the padding)
        const unsigned off = (col < dj * 8) ? (unsigned)(rowc * (dj * 8) + col) : 0u;
        const char *src = base + off;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(reinterpret_cast<char *>(dst) + 1024 * q),
                                         16, 0, 0);
      }
    }
  };
  if (blockIdx.x < nblocks) stage((int64_t)blockIdx.x * FB, xbuf);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int cur = 0;
#ifdef VCMI_ESTEP_PROF
  unsigned long long pt_[6] = {0, 0, 0, 0, 0, 0};     // probe build: s_memtime counts in A | barrier | softmax | barrier | B | barrier
#define VCMI_PT(i) { const unsigned long long t_ = __builtin_readcyclecounter(); pt_[i] += t_ - tl_; tl_ = t_; }
#else
#define VCMI_PT(i)
#endif
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x, cur ^= 1) {
#ifdef VCMI_ESTEP_PROF
    unsigned long long tl_ = __builtin_readcyclecounter();
#endif
    const int64_t f0 = blk * FB;
    const double *xs = xbuf + cur * XBUF;
    double gpre[kGamma ? 1 : FB / 4];         // PHASE 2: this lane's responsibilities of the block, fetched before the products
    if constexpr (kGamma) {
      // ---- step A: l[m][f] = c_m + sum_k W[m][k] Xe[k][f],  Xe = [x^2 ; x] ----
#pragma unroll
      for (int ft = 0; ft < FB / 16; ++ft) {
        if constexpr (SHARE) {
          if ((ft & (wpt - 1)) != (sub & (wpt - 1)) || (wpt > FB / 16 && sub >= FB / 16)) continue;     // wave-uniform
        }
        d4 acc = cin;
        nmfma += KS;
        const double *xr = xs + (16 * ft + lcol) * RSX + lgrp;
#pragma unroll
        for (int ks = 0; ks < KS / 2; ++ks) {
          const double x = xr[4 * ks];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x * x, wfrag[ks], acc, 0, 0, 0);
          if constexpr (C::SPLIT) {         // 160 registers hold W: keep the operand reads from running far ahead
            if ((ks & 3) == 3) __builtin_amdgcn_sched_barrier(0);
          }
        }
#pragma unroll
        for (int ks = 0; ks < KS / 2; ++ks) {
          const double x = xr[4 * ks];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, wfrag[KS / 2 + ks], acc, 0, 0, 0);
          if constexpr (C::SPLIT) {
            if ((ks & 3) == 3) __builtin_amdgcn_sched_barrier(0);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) lg[(16 * ft + 4 * r + lgrp) * RSG + 16 * tile + lcol] = acc[r];
      }
      VCMI_PT(0)
      __syncthreads();
      VCMI_PT(1)
      // ---- softmax over the 128 mixture slots of each frame.  16 lanes per frame, lane lcol owns slots lcol + 16 i:
      //      per instruction a 32-lane group touches 2 frame rows x 16 consecutive doubles, which with RSG == 16 mod 32
      //      is conflict-free (same pattern as step B's gamma reads) ----
      // the next block streams in from here on (issued in the phase with the lowest register pressure; it has the
      // softmax and step B to land)
      if (blk + gridDim.x < nblocks) stage((blk + gridDim.x) * FB, xbuf + (cur ^ 1) * XBUF);
#pragma unroll
      for (int ps = 0; ps < FB / 32; ++ps) {
        const int f = 32 * ps + 4 * wave + lgrp;
        double *row = lg + f * RSG + lcol;
        double v[C::MMAX / 16];
        double u = -INFINITY;
#pragma unroll
        for (int i = 0; i < C::MMAX / 16; ++i) {
          v[i] = (!SHARE || i < mtp) ? row[16 * i] : -INFINITY;          // slots of tiles that do not exist: gamma = 0
          u = fmax(u, v[i]);
        }
        int wtile = 0;                        // (kSortB) the first slot of this lane that attains its maximum
        if constexpr (kSortB) {
          const double ul = u;
#pragma unroll
          for (int i = C::MMAX / 16 - 1; i >= 0; --i) wtile = (v[i] == ul) ? i : wtile;
        }
        const double ulane = u;
        u = row16_max(u);                    // (DPP: no LDS round trips; fp64_exp.hpp)
        if constexpr (kSortB) {
          wtile = row16_min((ulane == u) ? wtile : 99);
          if (lcol == 0) fkey[f] = wtile < 8 ? wtile : 0;
        }
        // ---- refinement.  The GEMM form  x^2 (-1/2var) + x (mu/var) + c  cancels: with var down to min_covar = 1e-7 and
        //      |mu| ~ 10 its terms reach 1e9 and l carries an absolute error of ~1e-7.  That is harmless while one mixture
        //      owns the frame (gamma = 1 whatever l is) and wrong when several compete: the responsibilities inherit the
        //      error.  So when more than one mixture is within kRefine of the frame's maximum, exactly those are
        //      re-evaluated term by term, (x - mu)^2 / var summed over d, as the reference formula reads --
        //      unless the expanded form is provably good enough for the (frame, mixture): l at or above the mixture's threshold
        //      (estep_prep_kernel: an error bound of 1e-10 from the value itself; models with ordinary variances, the
        //      reference's trained ones among them, never re-evaluate anything).
        //      Round 6: the TEST costs nothing extra on the way -- a compare on the exps' own operand and one against the
        //      threshold per slot; "several compete" is read off the sum (s > 1: another mixture within ~36 nats) -- and the
        //      re-evaluation, with a second softmax of the frame, sits behind one wave-uniform branch.  (Before, every frame
        //      with competing mixtures -- every frame of real joint mel-cepstra -- walked its slots through LDS one by one to
        //      find nothing: ~150 of a pass's ~400 VALU instructions, each paid for in matrix-pipe time.)
        constexpr double kRefine = 36.0;     // e^-36 = 2e-16: a mixture further below the maximum cannot change a sum
        bool needl = false;                  // one of this lane's slots is within kRefine of the maximum and below its threshold
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < C::MMAX / 16; ++i) {
          const double dlt = v[i] - u;
          if (!SHARE || i < mtp) needl = needl || (dlt > -kRefine && v[i] < tthr[lcol + 16 * i]);
#if VCMI_ESTEP_EXP_SKIP
          // the 16 mixtures of slot group i are hopeless for all four frames of the pass (e^x = 0 below -745.2): no exp at all
          if (__builtin_amdgcn_ballot_w64(dlt > -745.2) == 0) {
            v[i] = 0.0;
            continue;
          }
#endif
          v[i] = vc_exp_tab(dlt, etab);   // 20 instructions against the 42 of exp(); -inf and < -745 give exactly 0
          s += v[i];
        }
        s = row16_sum(s);
        // PHASE 3 (one group of 128 of a larger model): a mixture that is alone near the top of ITS group may still compete
        // with one of another group, which this launch cannot see -- so every value within kRefine of the group's maximum is
        // made exact, the maximum itself included (a mixture within 36 nats of the frame's maximum over all groups is within
        // 36 nats of its own group's maximum): cross-group competition then sees exact log-densities too
        const bool need = needl && (PHASE == 3 || s > 1.0);
        if (__builtin_amdgcn_ballot_w64(need) != 0) {
          const double thr = u - kRefine;
          const double *xf = xs + f * RSX;
#pragma unroll 1
          for (int i = 0; i < mtp; ++i) {
            const double li = row[16 * i];           // (still the log-densities: the responsibilities are stored below)
            if (need && li > thr && li < tthr[lcol + 16 * i]) {
              const int m = lcol + 16 * i;
              const double *mp = refmu + (size_t)dj * m, *ip = refiv + (size_t)dj * m;
              double q = 0.0;
#pragma unroll 2
              for (int d = 0; d < dj; ++d) {
                const double df = xf[d] - mp[d];
                q = fma(df * df, ip[d], q);
              }
              row[16 * i] = refc[2 * m] - 0.5 * q;
            }
          }
          u = -INFINITY;
#pragma unroll
          for (int i = 0; i < C::MMAX / 16; ++i) {
            v[i] = (!SHARE || i < mtp) ? row[16 * i] : -INFINITY;
            u = fmax(u, v[i]);
          }
          u = row16_max(u);
          s = 0.0;
#pragma unroll
          for (int i = 0; i < C::MMAX / 16; ++i) {
            v[i] = vc_exp_tab(v[i] - u, etab);
            s += v[i];
          }
          s = row16_sum(s);
        }
        const bool livef = (f0 + f < N);
        // frames beyond N contribute gamma = 0; so does a slot group whose mixtures ALL have zero weight (every l = -inf:
        // u = -inf, s = 0 -- a 128-group of a padded model, M = 129 with w[129] = 0): gamma = 0 and log-sum-exp = -inf, not NaN
        // 1 / s, s in [1, 128]: the hardware's estimate and two Newton steps (none of the division's scaling / fix-up cases can occur)
        const double sc_ = s > 0.0 ? s : 1.0;
        double rq_ = __builtin_amdgcn_rcp(sc_);
        rq_ = fma(fma(-sc_, rq_, 1.0), rq_, rq_);
        rq_ = fma(fma(-sc_, rq_, 1.0), rq_, rq_);
        const double inv = (livef && s > 0.0) ? rq_ : 0.0;
#pragma unroll
        for (int i = 0; i < C::MMAX / 16; ++i)
          if (!SHARE || i < mtp) row[16 * i] = v[i] * inv;
        if constexpr (PHASE == 3) {
          if (lcol == 0 && livef) part[f0 + f] = u + log(s);      // the group's log-sum-exp of this frame
        } else {
          // log-likelihood: sum of u + log s over the frames.  log() is ~100 instructions and s lies in [1, 128], so the
          // s of a lane's frames are multiplied up (16 of them stay below 1e34) and ONE log is taken per eight blocks
          if (lcol == 0 && livef) {
            llacc += u;
            sprod *= s;
          }
        }
      }
      if constexpr (PHASE != 3) {
        if (++nprod == 8) {                   // (wave-uniform)
          llacc += log(sprod);
          sprod = 1.0;
          nprod = 0;
        }
      }
      VCMI_PT(2)
      __syncthreads();
      VCMI_PT(3)
      if constexpr (kSortB) {
        // counting sort of the block's FB frames by winning tile, every wave for itself (lane = frame; ballots + mbcnt):
        // fperm[position] = frame.  Stable, so the order -- and with it every sum -- is a function of the data alone.
        static_assert(FB == 64, "one lane per frame");
        const int k = fkey[lane];
        int base = 0, pos = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const unsigned long long bt = __builtin_amdgcn_ballot_w64(k == t);
          const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(bt >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bt, 0));
          pos = (k == t) ? base + below : pos;
          base += __builtin_popcountll(bt);
        }
        fperm[pos] = lane;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the wave's own LDS writes are visible to its reads below
      }
      if constexpr (PHASE == 1 || PHASE == 3) {  // responsibilities -> G, rows of 128, coalesced
#pragma unroll
        for (int i = 0; i < FB * C::MMAX / 512; ++i) {
          const int e = tid + 512 * i, f = e / C::MMAX, m = e - f * C::MMAX;
          if (f0 + f < N) G[(f0 + f) * C::MMAX + m] = (m < 16 * mtp) ? lg[f * RSG + m] : 0.0;
        }
      }
    } else {
      if (blk + gridDim.x < nblocks) stage((blk + gridDim.x) * FB, xbuf + (cur ^ 1) * XBUF);
#pragma unroll
      for (int ks = 0; ks < FB / 4; ++ks) {
        const int64_t f = f0 + 4 * ks + lgrp;
        gpre[ks] = (f < N) ? G[f * C::MMAX + 16 * tile + lcol] : 0.0;     // frames beyond N contribute gamma = 0
      }
    }
    // ---- step B: S[m][c] += sum_f gamma[f][m] Xe[f][c],  Xe = [x | x^2];  S0[m] += sum_f gamma[f][m] ----
    if constexpr (kStats) {
#pragma unroll kStepBUnroll
      for (int ks = 0; ks < FB / 4; ++ks) {
        if constexpr (SHARE) {
          if ((ks & (wpt - 1)) != sub) continue;             // wave-uniform: this tile's waves share the k-steps
        }
        const int f = kSortB ? fperm[4 * ks + lgrp] : 4 * ks + lgrp;
        double gm;
        if constexpr (PHASE == 0) gm = lg[f * RSG + 16 * tile + lcol];
        else gm = gpre[ks];
        // responsibilities that underflowed to exactly 0 (l_m more than 745 nats under the frame's maximum: the usual case
        // for all but a few of the 128 mixtures) add exactly nothing: when that holds for the tile's 16 mixtures on all
        // four frames of the k-step, its 2 NDT/2 products are skipped (wave-uniform; the statistics are bit-identical)
        if (__builtin_amdgcn_ballot_w64(gm != 0.0) == 0) continue;
        nmfma += NDT;
        const double *xr = xs + f * RSX + lcol;
#pragma unroll
        for (int j = 0; j < NDT / 2; ++j) {
          const double x = xr[16 * j];
          sacc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(gm, x, sacc[j], 0, 0, 0);
          sacc[NDT / 2 + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(gm, x * x, sacc[NDT / 2 + j], 0, 0, 0);
        }
        s0l += gm;
      }
    }
    VCMI_PT(4)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next block's LDS-DMA has landed
    __syncthreads();
    VCMI_PT(5)
  }
#ifdef VCMI_ESTEP_PROF
  if (blockIdx.x == 3 && (tid & 63) == 0)
    printf("estep prof wave %d: A %llu | bar %llu | softmax %llu | bar %llu | B %llu | bar %llu\n", wave, pt_[0], pt_[1], pt_[2], pt_[3], pt_[4], pt_[5]);
#endif
#undef VCMI_PT

  if (mfma_count && lane == 0) atomicAdd(mfma_count, (unsigned long long)nmfma);
  // ---- write this workgroup's partial statistics: rows m = 16 wave + lgrp + 4 r, cols = 16 j + lcol ----
  // row blockIdx.x * wpt + sub of the partial statistics: every mixture tile is written by the wave (tile, sub)
  double *P = part + ((size_t)blockIdx.x * wpt + sub) * plen;
  if constexpr (kStats) {
    s0l += __shfl_xor(s0l, 16);
    s0l += __shfl_xor(s0l, 32);
    if (lgrp == 0 && 16 * tile + lcol < M) P[16 * tile + lcol] = s0l;
    if (lane == 0 && tile == 0 && sub > 0) P[plen - 1] = 0.0;        // the log-likelihood travels in row sub = 0
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 16 * tile + 4 * r + lgrp;
      if (m < M) {
#pragma unroll
        for (int j = 0; j < NDT; ++j) {
          const int c = 16 * j + lcol;   // column of [x | x^2]
          if (c < DJ) {
            if (c < dj) P[M + (size_t)m * dj + c] = sacc[j][r];
          } else if (c - DJ < dj) {
            P[M + (size_t)M * dj + (size_t)m * dj + (c - DJ)] = sacc[j][r];
          }
        }
      }
    }
  }
  if constexpr (kGamma && PHASE != 3) {   // log-likelihood: fixed-order reduction inside the workgroup (thread 0: tile 0, sub 0)
    // (butterflies within a wave, then the eight waves in order: a fixed order; thread 0 walking 512 LDS entries took 14 us at
    // the end of every workgroup)
    llacc += log(sprod);
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) llacc += __shfl_xor(llacc, sh);
    if (lane == 0) red[wave] = llacc;
    __syncthreads();
    if (tid == 0) {
      double ll = 0.0;
      for (int i = 0; i < 8; ++i) ll += red[i];
      P[plen - 1] = ll;
    }
  }
}

}  // namespace vcmi
