// gmmmap.hip -- GMM joint-density mapping on MI355X (gfx950): the FP64 MFMA tile kernel of the batched fvconvert, posterior
// and argmax, the screen kernels (gmmmap_screen.hpp), their dispatch and the four device routines behind the C entry points.
// Around it: the kernels for dimensions without a tile instantiation are gmmmap_fallback.hip, the frame grouping is
// gmmmap_group.hip (grouping.hpp), the EM loop's on-device p(x) preparation is gmm_px_prep.hip, the device-group replicas and
// the C entry points are gmmmap_api.cpp.
// The host-side model preparation (factorisation, profile, the packers of every device image) is gmmmap_prepare.cpp;
// what its packers and these kernels must agree on (row tiling, issue order, stage layouts) is gmmmap_layout.hpp.
//
// Replaces, for whole (D,T) matrices at once:
//   GMMMap ctor / GMMMapParam / split_joint_gmm          reference src/gmmmap.jl:23-90
//   GaussianMixtureModel (Hermitian + Cholesky)          reference src/gmm.jl:8-20
//   fvconvert(g::GMMMap, x)                              reference src/gmmmap.jl:101-118
//   predict_proba / predict                              reference src/gmm.jl:24-58
//   vc(c::FrameByFrameConverter, fm)                     reference src/common.jl:7-26
//
// Math.  Per mixture m, prepared once on the host (gmmmap_prepare.cpp):
//   A_m = Syx_m inv(Sxx_m)              b_m  = muy_m - A_m mux_m
//   L_m L_m' = Hermitian(Sxx_m)         U_m  = inv(L_m)   (lower triangular)     cz_m = U_m mux_m
//   lc_m = log w_m - (D log 2pi + 2 sum_i log L_m[i,i]) / 2
// Per frame x:   z_m = U_m x - cz_m,  l_m = lc_m - |z_m|^2 / 2,  p = softmax(l),  y = sum_m p_m (A_m x + b_m).
// The softmax is evaluated online (running max + rescale), so no (M,T) posterior is ever stored by convert.
//
// MFMA kernel data layout: the 2*Dp rows [U_m ; A_m] (Dp = D rounded up to 4) are cut into 16-row tiles;
// D[16 rows x 16 frames] += W[16 rows x 4 k] * X[4 k x 16 frames] is one v_mfma_f64_16x16x4_f64.  U-only
// tiles skip the k-steps that are entirely above the diagonal.  Each mixture's operand fragments are stored
// in HBM in issue order, 64 lanes x 8 B per step, so the global->LDS stage is a straight copy and every
// ds_read_b64 is conflict-free.
#include "vcmi_common.hpp"
#include "gmmmap_handle.hpp"
#include "gmmmap_fallback.hpp"
#include "fp64_exp.hpp"
#include "grouping.hpp"
#include "gmmmap_rows.hpp"
#ifndef VCMI_CONVERT_PRIO
#define VCMI_CONVERT_PRIO 1        // s_setprio: 1 = a wave's stretches WITHOUT MFMAs (|z|^2, the test, the y update, the barrier) at high
                                   // priority, so that it is back in an MFMA stream sooner (+1..2 % on one box); 2 = the reverse; 0 = none
#endif
#include "gmmmap_screen.hpp"

#include <algorithm>
#include <cmath>

namespace vcmi {

// ------------------------------------------------------------------------------------------------
// MFMA tile kernel.  One wave owns FT tiles of 16 frames; a workgroup of WAVES waves shares the
// per-mixture operand block, double-buffered in LDS.
// MODE 0: convert (writes Y).  MODE 1: log-weighted densities l_m (writes LP (M,T)), no A tiles used.
// MODE 2: predict -- the 1-based index of the first maximum of l_m over m (src/gmm.jl:44-47) written as int64 to Y[frame];
// the (M,T) matrix never exists.  MODE 3: the same result from fragments stored tile by tile, last tile first, with an
// EXACT early exit: |z|^2 only grows as tiles are added, so once lc - |z partial|^2 / 2 <= runmax on all 16 frames of a
// frame tile, mixture m cannot be its first maximum and the remaining tiles are skipped.  The LAST rows of the Cholesky
// whitening carry the small conditional variances, i.e. most of a wrong mixture's distance: they go first.
// ------------------------------------------------------------------------------------------------
// PRUNE (MODE 0 only) -- three code shapes of the same arithmetic:
//   2  "peaked": everything the round-3 loop does (last whitening tile first, tests on the lane groups' shares, per-tile
//      branches around idle MFMAs) -- pays when almost every (tile, mixture) pair is decided out early;
//   1  "broad": every whitening tile of every mixture, ONE wave-uniform branch around the regression + softmax update of a
//      mixture that no frame of the wave's tiles gives a posterior above e^-prune -- the loop body is two straight blocks;
//   0  dense (prune = +inf): no test at all.
// In shapes 0 and 1 the weight e^(l - max) is formed BEFORE the regression tiles, so that its dependent chain issues in
// the shadow of their MFMAs instead of after them.
template <int DP, int FT, int WAVES, int MODE, int NBUF, int PRUNE = 2>
__global__ void __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(DP <= 40 ? (FT == 2 ? 3 : 4) : 2)))
gmmmap_mfma_kernel(const double *__restrict__ packed, int M, int D, const double *__restrict__ X, int64_t ldx,
                   int64_t T, double *__restrict__ Y, int64_t ldy, double prune, unsigned long long *__restrict__ nreg,
                   const int *__restrict__ perm, const int *__restrict__ gkey) {
  // perm / gkey (MODE 0, optional): frames GROUPED by (approximate) mixture -- position fr of the launch is frame perm[fr],
  // gkey[frame] its group -- see gmmmap_group.hip: a 16-frame tile then holds frames of one mixture, the workgroup starts
  // its mixture loop at that mixture, the running maximum is tight from the first iteration and the pruning removes (almost)
  // every other regression.  Frames are independent of each other, so the results do not depend on the grouping.
  using TL = Tiling<DP, MODE >= 1>;
  constexpr int KS = TL::KS, NT = TL::NT, NU = TL::NU, BLK = TL::BLK;
  constexpr int NTHREADS = WAVES * 64;
  constexpr int NV = BLK / 2 / NTHREADS;   // double2 copies per thread per block (BLK is a multiple of 1024)
  static_assert(BLK % (2 * NTHREADS) == 0, "block size must be a whole number of double2 per thread");
  extern __shared__ double smem[];                          // NBUF * BLK doubles
  // MODE 1: write-combining stage for the (T,M) log-density output.  A lane owns a frame and produces one value per
  // mixture iteration; written directly these are 8-byte stores 8*M bytes apart (PMC: WRITE_SIZE 4x the bytes of the
  // matrix).  Values of 8 consecutive mixtures are parked here and then leave as 64-byte rows.
  constexpr int LROW = 10;                                  // 8 values + pad: 16-byte aligned, conflict-free for 16 lanes
  __shared__ __attribute__((aligned(16))) double lstage[(MODE == 1) ? WAVES * FT * 16 * LROW : 2];
  __shared__ double etab[(MODE == 0 && PRUNE < 2) ? 64 : 1];   // 2^(j/64) for vc_exp_tab
  if constexpr (MODE == 0 && PRUNE < 2) {
    if (threadIdx.x < 64) etab[threadIdx.x] = kExp2Tab[threadIdx.x];   // (visible after the barrier that follows the first stage)
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);     // the same number in a scalar register (uniform address arithmetic)
  const unsigned lane_off = 16u * (unsigned)lane;               // this lane's 16 bytes of a 1 KB LDS-DMA wave instruction
  const int lcol = lane & 15;   // frame within a 16-frame tile (MFMA column)
  const int lgrp = lane >> 4;   // k within a k-step (operands) / row offset within a register group (results)
  const int64_t frame0 = ((int64_t)blockIdx.x * WAVES + wave) * (16 * FT);

  // B operands: xb[f][ks] = X[k = 4 ks + lgrp][frame = frame0 + 16 f + lcol], zero outside (D, T)
  double xb[FT][KS];
  int64_t frow[FT];              // the frame a tile column stands for (perm: grouped launch)
#pragma unroll
  for (int f = 0; f < FT; ++f) {
    const int64_t fr = frame0 + 16 * f + lcol;
    frow[f] = (MODE == 0 && perm != nullptr && fr < T) ? (int64_t)perm[fr] : fr;
    load_frame_row<KS>(X + (fr < T ? frow[f] : (int64_t)0) * ldx, fr < T, rows_as_lines(X, ldx, D, DP), D, lgrp, xb[f]);
  }
  // first mixture of the loop: the group of the workgroup's first frame (grouped launch), else 0
  int mfirst = 0;
  if (MODE == 0 && perm != nullptr) {
    const int64_t f0 = (int64_t)blockIdx.x * WAVES * (16 * FT);
    mfirst = (f0 < T) ? gkey[perm[f0]] : 0;
    mfirst = (mfirst >= 0 && mfirst < M) ? mfirst : 0;
  }

  int nreg_wave = 0;              // MODE 0: (tile, mixture) regressions this wave evaluated (diagnostic counter, see nreg)
  int nmfma_wave = 0;             // MODE 0: v_mfma_f64_16x16x4 instructions this wave issued (nreg[1]; wave-uniform scalar adds)
  unsigned tiles_in_range = 0;    // the wave's tiles that hold at least one frame < T
#pragma unroll
  for (int f = 0; f < FT; ++f)
    if (frame0 + 16 * f < T) tiles_in_range |= 1u << f;
  double yacc[FT][KS];
  double runmax[FT], den[FT];
  int bestm[FT];                  // MODE 2: runmax = the largest l_m so far, bestm = its (first) mixture
#pragma unroll
  for (int f = 0; f < FT; ++f) {
    bestm[f] = 0;
    runmax[f] = -INFINITY;
    den[f] = 0.0;
#pragma unroll
    for (int j = 0; j < KS; ++j) yacc[f][j] = 0.0;
  }

  // stage the first block
  {
    const double2 *src = reinterpret_cast<const double2 *>(packed + (size_t)mfirst * BLK);
    double2 *dst = reinterpret_cast<double2 *>(smem);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = tid + i * NTHREADS;
      dst[e] = src[e];
    }
  }
  __syncthreads();

  // (the constant address space makes a uniform-address load a scalar load; the blocks are read-only for the kernel)
  const __attribute__((address_space(4))) double *packed_c = (const __attribute__((address_space(4))) double *)packed;
  double lc_next = packed_c[(size_t)mfirst * BLK + TL::LC_OFF];      // (every mode; mfirst = 0 outside MODE 0)
#ifdef VCMI_CONVERT_PROF
  unsigned long long prof_barrier_ = 0;
  const unsigned long long prof_t0_ = __builtin_readcyclecounter();
#endif
#ifdef VCMI_CONVERT_PROF2
  // phase probe (s_memtime counts; reading it waits for the wave's outstanding LDS / scalar operations, which the phase
  // boundaries do anyway): [0] loop top -> lc known, [1] first part of the mixture (peaked: last whitening tile + test;
  // dense / broad: whitening + |z|^2), [2] the rest up to the barrier, [3] vmcnt + barrier
  unsigned long long pp_[4] = {0, 0, 0, 0};
  unsigned long long pt_ = __builtin_readcyclecounter();
#define VCMI_PP(i) { const unsigned long long n_ = __builtin_readcyclecounter(); pp_[i] += n_ - pt_; pt_ = n_; }
#else
#define VCMI_PP(i)
#endif
  // Two copies of the loop body, one per staging buffer (the inner loop is unrolled): the buffer's offset is then a
  // compile-time constant that goes into the immediate offsets of the LDS reads, instead of a run-time base that costs two or
  // three VALU address instructions at the start of every MFMA stream.
  // (Measured, one box: dense 5.10 -> 5.08 ms, peaked 1.700 -> 1.674; the broad shape spills four registers in this form and
  // loses 2 %: it keeps the single copy.)
  constexpr int UNR = (MODE == 0 && PRUNE == 1) ? 1 : 2;
  for (int mo = 0; mo < M; mo += UNR) {
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const int mi = mo + u;
    if (UNR > 1 && mi >= M) break;                                         // (odd M: wave-uniform)
    const int par = (UNR > 1) ? u : (mi & 1);
    const int m = (mfirst + mi < M) ? mfirst + mi : mfirst + mi - M;       // mixtures in rotated order (mfirst = 0: index order)
    const double *cur = smem + (NBUF == 2 ? par * BLK : 0);
    double2 *nxt = reinterpret_cast<double2 *>(smem + (NBUF == 2 ? (par ^ 1) * BLK : 0));
    // How block m+1 gets into LDS (unconditionally: the last iteration re-reads its own block, so the loop body has no
    // exec-mask branch).  Rounds 1-3 requested the whole block into registers here and stored it to LDS after the MFMA work:
    // the compiler sinks those loads down to the LDS stores (24 registers it does not have at 3 waves per SIMD), so the full
    // L2 latency stood in front of every barrier.  STAGE_DMA (two buffers): global_load_lds_dwordx4 -- 16 bytes per lane
    // straight into the other buffer, no registers; a wave instruction fills 1 KB; issued here, waited for (vmcnt) just
    // before the barrier.  The target buffer was last read in the previous iteration, before that iteration's barrier.
    // (A single buffer, NBUF = 1 -- blocks beyond 40 KB -- keeps the register path.)
#ifndef VCMI_CONVERT_STAGE
#define VCMI_CONVERT_STAGE 2
#endif
    constexpr bool STAGE_DMA = (VCMI_CONVERT_STAGE == 2 && NBUF == 2);
    double2 pre[STAGE_DMA ? 1 : NV];
    const int mn = (mi + 1 < M) ? ((m + 1 < M) ? m + 1 : 0) : m;
    if constexpr (STAGE_DMA) {
      // Addresses: a UNIFORM base (scalar registers, scalar arithmetic) plus one loop-invariant 32-bit lane offset.  Written
      // with per-lane pointers (base + 16 tid), every one of the NV instructions cost a 64-bit VALU add, a VALU add for the
      // LDS address and a v_readfirstlane to get it into M0 -- and a VALU instruction of any kind waits for the FP64 MFMAs of
      // the SIMD's other waves: the phase probe (-DVCMI_CONVERT_PROF2) showed loop top -> first MFMA taking as long as the 20
      // MFMAs of the peaked loop's first stage.
      // (The builtin does not select the scalar-base form -- it folds the lane offset into a per-lane 64-bit pointer again --
      // so the instruction is written out: M0 = LDS byte address of the wave's 1 KB, saddr = uniform global address,
      // vaddr = the lane's 16-byte offset.)
      const char *gbase = reinterpret_cast<const char *>(packed + (size_t)mn * BLK) + 1024 * wave_u;
      const unsigned lbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)(reinterpret_cast<char *>(nxt)) + 1024u * wave_u;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const char *ga = gbase + 16 * NTHREADS * i;
        const unsigned la = lbase + 16u * NTHREADS * i;
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(lane_off), "s"(ga), "s"(la) : "memory", "m0");
      }
      __builtin_amdgcn_sched_barrier(0);
    } else {
      const double2 *nsrc = reinterpret_cast<const double2 *>(packed + (size_t)mn * BLK);
#pragma unroll
      for (int i = 0; i < NV; ++i) pre[i] = nsrc[tid + i * NTHREADS];
    }

    // lc_m: a scalar load from the block's copy in global memory, requested one iteration ahead (MODE 0; a uniform address:
    // s_load, no VALU, no LDS round trip at the top of the iteration), compared as an integer (-inf = zero weight)
    double lc;
    // Where the NEXT lc is requested matters: an outstanding scalar load turns the compiler's s_waitcnt on LDS reads into
    // lgkmcnt(0) (scalar loads return out of order), and the barrier waits for it too.  So: right after the first stage's
    // |z|^2 arithmetic -- its LDS reads are done, ~30 VALU instructions and a branch follow -- (VCMI_LC_NEXT below).
    lc = lc_next;
    bool lcn_done = false;
#define VCMI_LC_NEXT                                             \
  {                                                              \
    lc_next = packed_c[(size_t)mn * BLK + TL::LC_OFF];           \
    lcn_done = true;                                             \
  }
    // the high word of -inf (lc is never NaN): a scalar compare
    const bool has_weight = (unsigned)((unsigned long long)__double_as_longlong(lc) >> 32) != 0xFFF00000u;
#ifdef VCMI_CONVERT_PROF2
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    VCMI_PP(0)
#endif
    if constexpr (MODE == 0 && PRUNE < 2) {
      if (has_weight) {
        d4 acc[FT][NT];
#pragma unroll
        for (int t = 0; t < NU; ++t) {
          d4 c;
#pragma unroll
          for (int r = 0; r < 4; ++r) c[r] = cur[TL::CINIT_OFF + 16 * t + 4 * r + lgrp];
#pragma unroll
          for (int f = 0; f < FT; ++f) acc[f][t] = c;
        }
        // ---------------- phase U: whitening tiles, z = U x - cz (k-step major: NU x FT independent chains) ----------------
        // the fragment of step s+1 is requested before the MFMAs of step s
        constexpr int NUS = TL::tile_off(NU);                 // fragments of the whitening phase
#if VCMI_CONVERT_PRIO == 1
        __builtin_amdgcn_s_setprio(0);
#elif VCMI_CONVERT_PRIO == 2
        __builtin_amdgcn_s_setprio(3);
#endif
        int s = 0;
        double a_cur = cur[lane];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
          for (int t = 0; t < NU; ++t) {
            if (ks < TL::steps(t)) {
              const double a = a_cur;
              ++s;
              if (s < NUS) a_cur = cur[s * 64 + lane];
#pragma unroll
              for (int f = 0; f < FT; ++f) acc[f][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xb[f][ks], acc[f][t], 0, 0, 0);
            }
          }
        }
        nmfma_wave += FT * NUS;
#if VCMI_CONVERT_PRIO == 1
        __builtin_amdgcn_s_setprio(3);      // A/B: the non-MFMA stretches of a wave at high priority
#elif VCMI_CONVERT_PRIO == 2
        __builtin_amdgcn_s_setprio(0);
#endif
        // |z|^2 per frame tile, then everything scalar about the softmax in the SELECTED layout when the wave has two tiles:
        // the even lane groups carry tile 0's l, running maximum and denominator, the odd ones tile 1's (psel picks) -- one
        // reduction, one test, one exp for both tiles
        double qv[FT];
#pragma unroll
        for (int f = 0; f < FT; ++f) {
          double qq = 0.0;
#pragma unroll
          for (int t = 0; t < NU; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (16 * t + 4 * r < DP) qq = fma(acc[f][t][r], acc[f][t][r], qq);
          }
          qv[f] = qq;
        }
        VCMI_LC_NEXT
        constexpr bool PAIRED = (FT == 2);
        double lsel;                                   // PAIRED: l of this lane's tile; else l of tile 0
        if constexpr (PAIRED) lsel = lc - 0.5 * sum_lane_groups_pair(qv[0], qv[1]);
        else lsel = lc - 0.5 * sum_lane_groups(qv[0]);
        VCMI_PP(1)
        bool go = true;
        if constexpr (PRUNE == 1) {
          // p_m <= e^(l_m - runmax): below e^-prune on every frame of the wave's tiles -> neither the regression nor the softmax
          // update can change y (the term is under the rounding error of those that are kept)
          go = __builtin_amdgcn_ballot_w64(lsel > runmax[0] - prune) != 0;
        }
        if (go) {
          nreg_wave += __builtin_popcount(tiles_in_range);
          nmfma_wave += FT * (TL::NSTEPS - NUS);
          // lazy rescale: only when some frame of the wave has a new maximum (wave-uniform; sc = 1 exactly for the others)
          if (__builtin_amdgcn_ballot_w64(lsel > runmax[0]) != 0) {
            const double nm = fmax(runmax[0], lsel);
            const double scs = vc_exp(runmax[0] - nm);
            den[0] *= scs;
            runmax[0] = nm;
            double sc[FT];
            if constexpr (PAIRED) unpair_lane_groups(scs, sc[0], sc[1]);
            else sc[0] = scs;
#pragma unroll
            for (int f = 0; f < FT; ++f) {
#pragma unroll
              for (int j = 0; j < KS; ++j) yacc[f][j] *= sc[f];
            }
          }
          double wg[FT];
          {
            const double e = vc_exp_tab(lsel - runmax[0], etab);
            den[0] += e;
            if constexpr (PAIRED) unpair_lane_groups(e, wg[0], wg[1]);
            else wg[0] = e;
          }
          // ---------------- phase A: regression tiles, E = A x + b ----------------
#if VCMI_CONVERT_PRIO == 1
          __builtin_amdgcn_s_setprio(0);
#elif VCMI_CONVERT_PRIO == 2
          __builtin_amdgcn_s_setprio(3);
#endif
#pragma unroll
          for (int t = NU; t < NT; ++t) {
            d4 c;
#pragma unroll
            for (int r = 0; r < 4; ++r) c[r] = cur[TL::CINIT_OFF + 16 * t + 4 * r + lgrp];
#pragma unroll
            for (int f = 0; f < FT; ++f) acc[f][t] = c;
          }
          int sa = NUS;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int t = NU; t < NT; ++t) {
              const double a = cur[sa * 64 + lane];
              ++sa;
#pragma unroll
              for (int f = 0; f < FT; ++f) acc[f][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xb[f][ks], acc[f][t], 0, 0, 0);
            }
          }
#if VCMI_CONVERT_PRIO == 1
          __builtin_amdgcn_s_setprio(3);
#elif VCMI_CONVERT_PRIO == 2
          __builtin_amdgcn_s_setprio(0);
#endif
#pragma unroll
          for (int f = 0; f < FT; ++f) {
#pragma unroll
            for (int t = NU - 1; t < NT; ++t) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int p0 = 16 * t + 4 * r;
                if (p0 >= DP && p0 < 2 * DP) {
                  const int j = (p0 - DP) / 4;
                  yacc[f][j] = fma(wg[f], acc[f][t][r], yacc[f][j]);
                }
              }
            }
          }
        }
      }
    } else
    if (has_weight) {   // zero-weight mixtures have posterior exactly 0 (wave-uniform branch)
      // ---------------- phase U: whitening tiles, z = U x - cz ----------------
      d4 acc[FT][NT];
      double q[FT];
      unsigned live = (1u << FT) - 1u;      // MODE 3: frame tiles of this wave that mixture m can still be the maximum of
      unsigned ulive = (1u << FT) - 1u;     // MODE 0: frame tiles whose whitening was completed (the others are decided: out)
      if constexpr (MODE == 3) {
        double qp[FT];
#pragma unroll
        for (int f = 0; f < FT; ++f) qp[f] = 0.0;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
          const int t = NU - 1 - i;
          if (!live) break;
          d4 c;
#pragma unroll
          for (int r = 0; r < 4; ++r) c[r] = cur[TL::CINIT_OFF + 16 * t + 4 * r + lgrp];
#pragma unroll
          for (int f = 0; f < FT; ++f) acc[f][t] = c;
#pragma unroll
          for (int ks = 0; ks < TL::steps(t); ++ks) {
            const double a = cur[(TL::rtile_off(i) + ks) * 64 + lane];
#pragma unroll
            for (int f = 0; f < FT; ++f)
              if (live >> f & 1u) acc[f][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xb[f][ks], acc[f][t], 0, 0, 0);
          }
#pragma unroll
          for (int f = 0; f < FT; ++f) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (16 * t + 4 * r < DP) qp[f] = fma(acc[f][t][r], acc[f][t][r], qp[f]);
          }
          if (i + 1 < NU) {
#pragma unroll
            for (int f = 0; f < FT; ++f) {
              if (!(live >> f & 1u)) continue;
              double qq = qp[f];
              qq = sum_lane_groups(qq);
              if (__builtin_amdgcn_ballot_w64(lc - 0.5 * qq > runmax[f]) == 0) live &= ~(1u << f);
            }
          }
        }
        VCMI_LC_NEXT
#pragma unroll
        for (int f = 0; f < FT; ++f) {
          double qq = qp[f];
          qq = sum_lane_groups(qq);
          q[f] = qq;
        }
      } else if constexpr (MODE == 0 && (TL::NU > 1)) {
        // fvconvert: the LAST whitening tile first (it spans all k-steps and carries the rows with the small conditional
        // variances, i.e. most of a wrong mixture's distance).  Its share of |z|^2 alone usually puts the mixture e^-prune
        // under every frame's running maximum -- certainly on grouped frames, where the maximum is the winner's from the
        // first iteration -- and then the other whitening tiles of this mixture are not computed at all (tested on the lane
        // groups' shares, no cross-lane sum; wave-uniform per frame tile).  Every tile keeps its own accumulation order.
        constexpr int TLAST = NU - 1;
        {
          // (round 4) the last tile's KS operand fragments are all requested before its first MFMA -- the compiler's order was
          // read, wait, FT MFMAs, read, wait, ...: an LDS round trip per k-step pair in a stage of only FT * KS MFMAs -- and
          // the other tiles' initial values are read only when they are needed (below)
          d4 c;
#pragma unroll
          for (int r = 0; r < 4; ++r) c[r] = cur[TL::CINIT_OFF + 16 * TLAST + 4 * r + lgrp];
#pragma unroll
          for (int f = 0; f < FT; ++f) acc[f][TLAST] = c;
          double afr[KS];
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) afr[ks] = cur[TL::ufrag_pos(ks, TLAST) * 64 + lane];
          __builtin_amdgcn_sched_barrier(0);       // (the scheduler sinks the reads back to their MFMAs otherwise)
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int f = 0; f < FT; ++f) acc[f][TLAST] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[ks], xb[f][ks], acc[f][TLAST], 0, 0, 0);
          }
        }
        nmfma_wave += FT * KS;
        VCMI_LC_NEXT
        unsigned und = (1u << FT) - 1u;        // frame tiles on which the mixture is still undecided
#pragma unroll
        for (int f = 0; f < FT; ++f) {
          double qq = 0.0;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (16 * TLAST + 4 * r < DP) qq = fma(acc[f][TLAST][r], acc[f][TLAST][r], qq);
          q[f] = qq;
          if (prune < 1e300) {
            const unsigned long long u = __builtin_amdgcn_ballot_w64(lc - 0.5 * qq > runmax[f] - prune);
            if ((u & (u >> 16) & (u >> 32) & (u >> 48) & 0xffffull) == 0) und &= ~(1u << f);
          }
        }
        ulive = und;
        VCMI_PP(1)
        if (und) {
          nmfma_wave += __builtin_popcount(und) * (TL::tile_off(NU) - KS);
#pragma unroll
          for (int t = 0; t < TLAST; ++t) {
            d4 c;
#pragma unroll
            for (int r = 0; r < 4; ++r) c[r] = cur[TL::CINIT_OFF + 16 * t + 4 * r + lgrp];
#pragma unroll
            for (int f = 0; f < FT; ++f) acc[f][t] = c;
          }
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int t = 0; t < TLAST; ++t) {
              if (ks < TL::steps(t)) {
                const double a = cur[TL::ufrag_pos(ks, t) * 64 + lane];
#pragma unroll
                for (int f = 0; f < FT; ++f)
                  if (FT == 1 || (und >> f & 1u)) acc[f][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xb[f][ks], acc[f][t], 0, 0, 0);
              }
            }
          }
#pragma unroll
          for (int f = 0; f < FT; ++f) {
            double qq = q[f];
#pragma unroll
            for (int t = 0; t < TLAST; ++t) {
#pragma unroll
              for (int r = 0; r < 4; ++r) qq = fma(acc[f][t][r], acc[f][t][r], qq);
            }
            q[f] = qq;                         // still the lane group's share (see the pruning test below)
          }
        }
      } else {
#pragma unroll
      for (int t = 0; t < NU; ++t) {
        d4 c;
#pragma unroll
        for (int r = 0; r < 4; ++r) c[r] = cur[TL::CINIT_OFF + 16 * t + 4 * r + lgrp];
#pragma unroll
        for (int f = 0; f < FT; ++f) acc[f][t] = c;
      }
      int s = 0;
      if (MODE == 0) nmfma_wave += FT * TL::tile_off(NU);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
        for (int t = 0; t < NU; ++t) {
          if (ks < TL::steps(t)) {
            const double a = cur[s * 64 + lane];
            ++s;
#pragma unroll
            for (int f = 0; f < FT; ++f) acc[f][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xb[f][ks], acc[f][t], 0, 0, 0);
          }
        }
      }
      VCMI_LC_NEXT
#pragma unroll
      for (int f = 0; f < FT; ++f) {
        double qq = 0.0;
#pragma unroll
        for (int t = 0; t < NU; ++t) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (16 * t + 4 * r < DP) qq = fma(acc[f][t][r], acc[f][t][r], qq);
          }
        }
        if (MODE == 2 || (MODE == 1 && FT != 2)) {   // (MODE 0 reduces over the four lane groups only when it has to: see below;
          qq = sum_lane_groups(qq);                  //  MODE 1 with two tiles: both in one exchange, below)
        }
        q[f] = qq;
      }
      }

      if (MODE == 1) {
        // log-weighted density of mixture m for the wave's frames.  Two tiles: ONE exchange sequence sums both (the even lane
        // groups end with tile 0's |z|^2, the odd ones with tile 1's) and lane groups 0 and 1 write their tile's value
        if constexpr (FT == 2) {
          const double lsel = lc - 0.5 * sum_lane_groups_pair(q[0], q[1]);
          if (lgrp < 2) lstage[((wave * FT + lgrp) * 16 + lcol) * LROW + (m & 7)] = lsel;
        } else if (lgrp == 0) {
#pragma unroll
          for (int f = 0; f < FT; ++f) lstage[((wave * FT + f) * 16 + lcol) * LROW + (m & 7)] = lc - 0.5 * q[f];
        }
      } else if (MODE == 2 || MODE == 3) {
#pragma unroll
        for (int f = 0; f < FT; ++f) {
          if (MODE == 3 && !(live >> f & 1u)) continue;     // l_m <= runmax on the whole tile: not its first maximum
          const double l = lc - 0.5 * q[f];
          if (l > runmax[f]) {          // strict: the first maximum wins, as in posterior_finish_kernel<1>
            runmax[f] = l;
            bestm[f] = m;
          }
        }
      } else {
        // Which of the wave's frame tiles can mixture m still contribute to?  p_m <= e^(l_m - runmax) for every frame, so
        // when l_m < runmax - prune for all 16 frames of a tile, its posterior there is below e^-prune (default e^-46 =
        // 1e-20, under the rounding error of the other terms) and neither the regression tiles A_m x + b_m nor the
        // softmax update can change y: both are skipped for that tile (wave-uniform).  prune = +inf keeps the dense loop.
        // q[f] still holds each lane GROUP's share of |z|^2 (lane = 16 group + frame).  |z|^2 is at least any one share, so a
        // frame is already out when one of its four lanes says so: only tiles with a frame that no single share rules out pay
        // for the cross-lane sum (two LDS round trips) -- for a wrong mixture every share is enormous.
        unsigned active = 0;
#pragma unroll
        for (int f = 0; f < FT; ++f) {
          if (!(ulive >> f & 1u)) continue;     // decided on the last tile's share alone
          if (prune < 1e300) {                  // (the dense loop, prune = +inf, has nothing to decide)
            const unsigned long long undecided = __builtin_amdgcn_ballot_w64(lc - 0.5 * q[f] > runmax[f] - prune);
            if ((undecided & (undecided >> 16) & (undecided >> 32) & (undecided >> 48) & 0xffffull) == 0) continue;
          }
          double qq = q[f];
          qq = sum_lane_groups(qq);
          q[f] = qq;
          if (__builtin_amdgcn_ballot_w64(lc - 0.5 * qq > runmax[f] - prune) != 0) active |= 1u << f;
        }
        if (MODE == 0) nreg_wave += __builtin_popcount(active & tiles_in_range);
        if (active) {
          if (MODE == 0) nmfma_wave += __builtin_popcount(active) * (TL::NSTEPS - TL::tile_off(NU));
          // ---------------- phase A: regression tiles, E = A x + b (wave-uniform branches around an idle tile's MFMAs) ----------------
          int sa = TL::tile_off(NU);
#pragma unroll
          for (int t = NU; t < NT; ++t) {
            d4 c;
#pragma unroll
            for (int r = 0; r < 4; ++r) c[r] = cur[TL::CINIT_OFF + 16 * t + 4 * r + lgrp];
#pragma unroll
            for (int f = 0; f < FT; ++f) acc[f][t] = c;
          }
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int t = NU; t < NT; ++t) {
              const double a = cur[sa * 64 + lane];
              ++sa;
#pragma unroll
              for (int f = 0; f < FT; ++f)
                if (FT == 1 || (active >> f & 1u)) acc[f][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xb[f][ks], acc[f][t], 0, 0, 0);
            }
          }
          // online softmax update:  y <- y * e^(old-new) + e^(l-new) * E
#pragma unroll
          for (int f = 0; f < FT; ++f) {
            if (FT > 1 && !(active >> f & 1u)) continue;
            const double l = lc - 0.5 * q[f];
#ifndef VCMI_LAZY
#define VCMI_LAZY 1
#endif
            if (!VCMI_LAZY || __builtin_amdgcn_ballot_w64(l > runmax[f]) != 0) {   // wave-uniform: some frame has a new maximum
              const double nm = fmax(runmax[f], l);
              const double sc = vc_exp(runmax[f] - nm);
              den[f] *= sc;
              runmax[f] = nm;
#pragma unroll
              for (int j = 0; j < KS; ++j) yacc[f][j] *= sc;
            }
            const double wg = vc_exp(l - runmax[f]);
            den[f] += wg;
#pragma unroll
            for (int t = NU - 1; t < NT; ++t) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int p0 = 16 * t + 4 * r;
                if (p0 >= DP && p0 < 2 * DP) {
                  const int j = (p0 - DP) / 4;
                  yacc[f][j] = fma(wg, acc[f][t][r], yacc[f][j]);
                }
              }
            }
          }
        }
      }
    }

    else if (MODE == 1 && lgrp == 0) {
#pragma unroll
      for (int f = 0; f < FT; ++f) lstage[((wave * FT + f) * 16 + lcol) * LROW + (m & 7)] = -INFINITY;
    }
    if (MODE == 1 && ((m & 7) == 7 || m == M - 1)) {
      // flush mixtures m0..m of the wave's FT*16 frames: lane = (frame, half row) -> 32 contiguous bytes each
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the wave's own ds_writes above have landed
      const int m0 = m & ~7, nv = m - m0 + 1;
#pragma unroll
      for (int i = 0; i < (FT * 16 * 2 + 63) / 64; ++i) {
        const int slot = lane + 64 * i, fl = slot >> 1, h = slot & 1;
        if (fl < FT * 16) {
          const int64_t fr = frame0 + fl;
          const double *row = &lstage[(wave * FT * 16 + fl) * LROW + 4 * h];
          double *dst = Y + fr * ldy + m0 + 4 * h;
          if (fr < T) {
            if (nv == 8 && ((ldy | m0) & 1) == 0) {
              const double2 a = *reinterpret_cast<const double2 *>(row), b2 = *reinterpret_cast<const double2 *>(row + 2);
              *reinterpret_cast<double2 *>(dst) = a;
              *reinterpret_cast<double2 *>(dst + 2) = b2;
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (4 * h + j < nv) dst[j] = row[j];
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // reads done before the next group's ds_writes reuse the rows
    }

    if (!lcn_done) lc_next = packed_c[(size_t)mn * BLK + TL::LC_OFF];       // (e.g. a mixture without weight: nothing ran above)
    if (NBUF == 1) __syncthreads();   // single buffer: everyone is done reading before it is overwritten
    VCMI_PP(2)
#ifdef VCMI_CONVERT_PROF
    const unsigned long long tb0_ = __builtin_readcyclecounter();
#endif
    if constexpr (STAGE_DMA) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) nxt[tid + i * NTHREADS] = pre[i];
    }
    __syncthreads();
#ifdef VCMI_CONVERT_PROF
    prof_barrier_ += __builtin_readcyclecounter() - tb0_;      // probe build: cycles between arriving at the barrier and leaving it
#endif
    VCMI_PP(3)
  }
  }
#undef VCMI_LC_NEXT
#ifdef VCMI_CONVERT_PROF2
  if (MODE == 0 && blockIdx.x == 1000 && lane == 0)
    printf("convert prof shape %d wave %d: top %llu | first %llu | rest %llu | barrier %llu (s_memtime counts over %d mixtures)\n", PRUNE, wave, pp_[0],
           pp_[1], pp_[2], pp_[3], M);
#endif
#undef VCMI_PP

  if (MODE == 2 || MODE == 3) {
    if (lgrp == 0) {
#pragma unroll
      for (int f = 0; f < FT; ++f) {
        const int64_t fr = frame0 + 16 * f + lcol;
        if (fr < T) reinterpret_cast<int64_t *>(Y)[fr] = bestm[f] + 1;
      }
    }
  }
  if (MODE == 0) {
    if (nreg && lane == 0) {
#ifdef VCMI_CONVERT_PROF
      // probe build: the counters carry s_memtime counts instead -- [0] waiting at the loop's barrier, [1] the whole loop
      atomicAdd(nreg, prof_barrier_);
      atomicAdd(nreg + 1, __builtin_readcyclecounter() - prof_t0_);
#else
      atomicAdd(nreg, (unsigned long long)nreg_wave);
      atomicAdd(nreg + 1, (unsigned long long)nmfma_wave);
#endif
    }
    if constexpr (PRUNE < 2 && FT == 2) {        // the dense / broad loops kept the denominators in the selected layout
      const double ds = den[0];
      unpair_lane_groups(ds, den[0], den[1]);
    }
#pragma unroll
    for (int f = 0; f < FT; ++f) {
      const int64_t fr = frame0 + 16 * f + lcol;
      const double inv = 1.0 / den[f];
      double yo[KS];
#pragma unroll
      for (int j = 0; j < KS; ++j) yo[j] = yacc[f][j] * inv;
      store_frame_row<KS>(Y + (fr < T ? frow[f] : (int64_t)0) * ldy, fr < T, rows_as_lines(Y, ldy, D, DP), D, lgrp, yo);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------
template <int DP, int MODE, int FTV, int WV, int PRUNE = 2>
static int launch_mfma(const vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy,
                       hipStream_t st, const int *perm = nullptr, const int *gkey = nullptr) {
  constexpr int FT = (MODE >= 1) ? 2 : FTV;
  constexpr int WAVES = WV;
  using TL = Tiling<DP, MODE >= 1>;
  // double-buffer the per-mixture block when two copies fit in half of the CU's 160 KiB LDS
  // (eight-wave workgroups -- one per CU -- take two buffers whenever they fit the CU's LDS at all)
  constexpr int NBUF = (2 * (size_t)TL::BLK * sizeof(double) <= (WAVES == 8 ? 156 : 80) * 1024) ? 2 : 1;
  const size_t shmem = NBUF * (size_t)TL::BLK * sizeof(double);
  auto kern = gmmmap_mfma_kernel<DP, FT, WAVES, MODE, NBUF, PRUNE>;
  static std::atomic<bool> attr_done[64];
  VCMI_TRY(set_max_dynamic_lds(kern, shmem, attr_done));
  const int64_t per_wg = (int64_t)16 * FT * WAVES;
  const int64_t blocks = (T + per_wg - 1) / per_wg;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(WAVES * 64), shmem, st, MODE == 3 ? g->packedU2.p : (MODE >= 1 ? g->packedU.p : g->packed.p), g->M,
                     g->D, dX, ldx, T, dY, ldy, g->prune, MODE == 0 ? g->prune_count.p : nullptr, MODE == 0 ? perm : nullptr,
                     MODE == 0 ? gkey : nullptr);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// Calls of up to this many frames do not fill the chip with 128-frame workgroups (2000 frames: 16 of 256 CUs, each walking
// all the mixtures for two frame tiles per wave): they run ONE frame tile per wave -- twice the workgroups, half the loop
// each.  Device-resident call of 2000 frames, D = 40, M = 64: 224 -> 127 us (the reference's 32-mixture model: 118 -> 79;
// one frame: 129 -> 83).  Grouping such calls (three more launches) does not pay: tools/small_T_sweep.py.
static constexpr int64_t kSmallCallFrames = 32768;

#ifndef VCMI_CONVERT_FT
#define VCMI_CONVERT_FT 2          // frame tiles per wave and waves per workgroup of the D <= 48 convert kernels (A/B builds)
#endif
#ifndef VCMI_CONVERT_WAVES
#define VCMI_CONVERT_WAVES 4
#endif
// (the arg-max kernel, MODE 3, takes the eight waves as well: 3.48 -> 3.25 ms per 512k frames at D = 80; the log-density kernel,
// MODE 1, gains nothing from them -- its two four-wave workgroups per CU already fill the register file: 3.87 / 3.85 ms)
#ifndef VCMI_WIDE_ALL_MODES
#define VCMI_WIDE_ALL_MODES 0
#endif
#ifndef VCMI_CONVERT_WAVES_WIDE
// Waves per workgroup of the fvconvert kernels beyond D = 48 (one frame tile per wave).  A mixture's block is 46 KB (DP = 52) to
// 102 KB (DP = 80) there, so a CU holds ONE or two workgroups: with four waves that was four to eight waves per CU, each
// workgroup streaming the whole model through LDS for its 64 frames.  Eight waves share a block (and two buffers where they
// fit: DP <= 72): 5e5 frames, M = 64: D = 56 8.06 -> 3.16 ms, D = 64 8.50 -> 3.34, D = 72 15.1 -> 4.54, D = 80 20.7 -> 10.1
// (tools/efficiency_sweep.py; A/B: -DVCMI_CONVERT_WAVES_WIDE=4).
#define VCMI_CONVERT_WAVES_WIDE 8
#endif
template <int MODE, int PRUNE = 2>
static int dispatch_mfma(const vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy,
                         hipStream_t st, const int *perm = nullptr, const int *gkey = nullptr) {
  if (MODE == 0 && g->DP <= 48 && T <= kSmallCallFrames && !debug_flag(kDbgConvertWideTiles)) {     // one frame tile per wave: twice the workgroups, half the loop each
    switch (g->DP) {
#define VCMI_CASE(DPV) \
  case DPV: return launch_mfma<DPV, MODE, 1, 4, PRUNE>(g, dX, ldx, T, dY, ldy, st, perm, gkey);
      VCMI_TILE_DIMS_48(VCMI_CASE)
#undef VCMI_CASE
      default: break;
    }
  }
  switch (g->DP) {
#define VCMI_CASE(DPV) \
  case DPV: return launch_mfma<DPV, MODE, ((DPV) <= 48 ? VCMI_CONVERT_FT : 1), ((DPV) == 40 && MODE == 0 ? VCMI_CONVERT_WAVES : ((DPV) > 48 && (MODE == 0 || MODE == 3 || VCMI_WIDE_ALL_MODES) ? VCMI_CONVERT_WAVES_WIDE : 4)), PRUNE>(g, dX, ldx, T, dY, ldy, st, perm, gkey);
    VCMI_TILE_DIMS(VCMI_CASE)
#undef VCMI_CASE
    default: return fail(VCMI_ERR_ARG, "no MFMA instantiation for padded dimension %d", g->DP);
  }
}

static bool use_mfma(const vcmi_gmmmap *g) {
  if (g->kernel_choice == 1) return false;
  return gmmmap_has_mfma(g->DP);
}

template <int DP, int FT, bool B16 = false>
static int launch_screen(const vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy, hipStream_t st,
                         const int *perm, const int *gbase) {
  constexpr int WAVES = 4;
  using TL = Tiling<DP, false>;
  constexpr int STG = B16 ? screen16_stage_doubles(DP) : screen_stage_doubles(DP);
  constexpr int BUF = (TL::BLK > STG) ? TL::BLK : STG;
  const size_t shmem = 2 * (size_t)BUF * sizeof(double);
  auto kern = gmmmap_screen_kernel<DP, FT, WAVES, B16>;
  static std::atomic<bool> attr_done[64];
  VCMI_TRY(set_max_dynamic_lds(kern, shmem, attr_done));
  const int64_t per_wg = (int64_t)16 * FT * WAVES;
  hipLaunchKernelGGL(kern, dim3((unsigned)((T + per_wg - 1) / per_wg)), dim3(WAVES * 64), shmem, st, g->packed.p, B16 ? g->packedQ16.p : g->packedQ.p, g->screen_rpm,
                     g->M, g->D, dX, ldx, T, dY, ldy, g->prune, g->prune_count.p, perm, gbase, B16 ? g->packedQ2.p : nullptr,
                     g->radius_on && !debug_flag(kDbgScreenNoRadius) ? g->lmin.p : nullptr);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}
static int dispatch_screen(const vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy, hipStream_t st,
                           const int *perm, const int *gbase) {
  const bool narrow = T <= kSmallCallFrames && !debug_flag(kDbgConvertWideTiles);     // one frame tile per wave, as dispatch_mfma
  // the screen on the BF16 matrix pipe (certified bound from split operands) where it exists: four rows per mixture, DP <= 40
  if (g->packedQ16.p && g->packedQ2.p && g->screen_rpm == 4 && screen16_has(g->DP) && !debug_flag(kDbgScreenFp64)) {
    switch (g->DP) {
#define VCMI_CASE(DPV) \
  case DPV: return narrow ? launch_screen<DPV, 1, true>(g, dX, ldx, T, dY, ldy, st, perm, gbase) : launch_screen<DPV, 2, true>(g, dX, ldx, T, dY, ldy, st, perm, gbase);
      VCMI_TILE_DIMS_40(VCMI_CASE)
#undef VCMI_CASE
      default: break;
    }
  }
  switch (g->DP) {
#define VCMI_CASE(DPV) \
  case DPV: return narrow ? launch_screen<DPV, 1>(g, dX, ldx, T, dY, ldy, st, perm, gbase) : launch_screen<DPV, 2>(g, dX, ldx, T, dY, ldy, st, perm, gbase);
    VCMI_TILE_DIMS_48(VCMI_CASE)
#undef VCMI_CASE
    default: return fail(VCMI_ERR_ARG, "no screening kernel for padded dimension %d", g->DP);
  }
}

// predict on grouped frames with the four-row screen (gmmmap_screen_argmax_kernel): every padded dimension of the tile kernel
template <int DP>
static int launch_screen_argmax(const vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, int64_t *didx, hipStream_t st,
                                const int *perm, const int *gbase) {
  constexpr int WAVES = 4;
  using TL = Tiling<DP, true>;
  constexpr int BUF = (TL::BLK > screen_stage_doubles(DP)) ? TL::BLK : screen_stage_doubles(DP);
  const size_t shmem = 2 * (size_t)BUF * sizeof(double);
  auto kern = gmmmap_screen_argmax_kernel<DP, WAVES>;
  static std::atomic<bool> attr_done[64];
  VCMI_TRY(set_max_dynamic_lds(kern, shmem, attr_done));
  const int64_t per_wg = (int64_t)32 * WAVES;
  hipLaunchKernelGGL(kern, dim3((unsigned)((T + per_wg - 1) / per_wg)), dim3(WAVES * 64), shmem, st, g->packedU.p, g->packedQA.p, g->M, g->D,
                     dX, ldx, T, didx, perm, gbase);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}
static int dispatch_screen_argmax(const vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, int64_t *didx, hipStream_t st,
                                  const int *perm, const int *gbase) {
  switch (g->DP) {
#define VCMI_CASE(DPV) \
  case DPV: return launch_screen_argmax<DPV>(g, dX, ldx, T, didx, st, perm, gbase);
    VCMI_TILE_DIMS(VCMI_CASE)
#undef VCMI_CASE
    default: return fail(VCMI_ERR_ARG, "no screening kernel for padded dimension %d", g->DP);
  }
}

static constexpr double kScreenArgmaxFrac = 0.10;      // predict: screened arg-max when at most this fraction of the mixtures survives the screen
static constexpr double kBroadModelFrac = 0.35;
// shape 3 pays while the survivors of the four-row screen stay few: a survivor costs its workgroup a block DMA and a barrier,
// and a whole mixture (42 MFMA steps at D = 40) every wave one of whose own frames let it through (the other waves skip it: the
// MFMA count at nreg[1] no longer holds their 22 whitening steps); a screened mixture 2.5 -- against the 10 of shape 2's
// last-tile test
static constexpr double kScreenModelFrac = 0.05;
// Which loop shape converts with this handle (gmmmap_mfma_kernel's PRUNE): 2 "peaked" when, for the model's own frames, the
// last whitening tile's share of |z|^2 alone puts most mixtures e^-prune under the best one (model.undecided, estimated
// once by profile_model(), gmmmap_prepare.cpp: 0.02 on the SURVEY 8d synthetic models) -- the loop that looks at that tile first then skips the other
// whitening tiles; 1 "broad" otherwise (every whitening tile is needed anyway: the straight loop is faster).
static int convert_shape(const vcmi_gmmmap *g) {
  const bool can_screen = screen_has_kernel(g->DP) && g->M <= 1024 && g->packedQ.p != nullptr;
  if (debug_flag(kDbgConvertShapeBroad)) return 1;
  if (debug_flag(kDbgConvertShapePeaked)) return 2;
  if (debug_flag(kDbgConvertShapeScreened) && can_screen) return 3;
  if (can_screen && g->model_undecided4_frac <= kScreenModelFrac) return 3;     // (grouped calls only: see gmmmap_convert_device)
  return g->model.undecided > kBroadModelFrac ? 1 : 2;
}

// what vcmi_gmmmap_convert_plan reports as the shape: -1 no tile kernel, 0 dense (prune = +inf), else convert_shape
int gmmmap_convert_plan_shape(const vcmi_gmmmap *g) { return !use_mfma(g) ? -1 : (!(g->prune < 1e300) ? 0 : convert_shape(g)); }

// convert on device pointers
int gmmmap_convert_device(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy,
                          hipStream_t st) {
  if (T == 0) return VCMI_OK;
  if (g->kernel_choice == 2 && !gmmmap_has_mfma(g->DP))
    return fail(VCMI_ERR_ARG, "MFMA kernel forced but dimension %d has no instantiation", g->D);
  if (use_mfma(g)) {
    // frames grouped by their nearest source mean first (gmmmap_group.hip): worth its two small kernels from a
    // few thousand frames on; the prune = +inf (dense) setting has nothing to gain from it
    if (can_group(g, T) && g->prune < 1e300 && !debug_flag(kDbgConvertNoGrouping)) {
      int *key = nullptr, *perm = nullptr, *gbase = nullptr;
      VCMI_TRY(launch_grouping(g, dX, ldx, T, st, &key, &perm, &gbase));
      const int shape = convert_shape(g);
      const int rc = shape == 3 ? dispatch_screen(g, dX, ldx, T, dY, ldy, st, perm, gbase)
                   : shape == 1 ? dispatch_mfma<0, 1>(g, dX, ldx, T, dY, ldy, st, perm, key)
                                : dispatch_mfma<0, 2>(g, dX, ldx, T, dY, ldy, st, perm, key);
      (void)g->grp_order.leave(st);
      return rc;
    }
    if (!(g->prune < 1e300) && !debug_flag(kDbgConvertShapePeaked)) return dispatch_mfma<0, 0>(g, dX, ldx, T, dY, ldy, st);
    // (frames in the caller's order: the screen of shape 3 needs the tight running maximum of grouped frames -> shape 2)
    return convert_shape(g) == 1 ? dispatch_mfma<0, 1>(g, dX, ldx, T, dY, ldy, st) : dispatch_mfma<0, 2>(g, dX, ldx, T, dY, ldy, st);
  }
  if (g->kernel_choice != 1 && g->At.p && g->D > 16 && g->D <= 160) {
    // no tile-kernel instantiation (80 < padded D <= 160, or a padded dimension outside its list): MFMA log-densities
    // (logdens_tiled_kernel) + softmax / regression over the mixtures that matter, in chunks that bound the (T,M) scratch
    const int64_t chunk = std::max<int64_t>(4096, ((int64_t)1 << 24) / std::max(g->M, 1));
    StreamOrderScope use(g->grp_order, st);       // scratch_lp is the handle's, like the grouping buffers: one order for both
    VCMI_TRY(use.status());
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
      const int64_t n = std::min(chunk, T - t0);
      VCMI_TRY(g->scratch_lp.reserve((size_t)std::min(chunk, T) * g->M));
      VCMI_TRY(gmmmap_logdens_device(g, dX + t0 * ldx, ldx, n, g->scratch_lp.p, st));
      VCMI_TRY(convert_from_logdens_launch(g, g->scratch_lp.p, dX + t0 * ldx, ldx, n, dY + t0 * ldy, ldy, st));
    }
    return VCMI_OK;
  }
  return gmmmap_generic_launch(g, 0, dX, ldx, T, dY, ldy, st);
}

// log-weighted densities (M,T) on device pointers
int gmmmap_logdens_device(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dLP, hipStream_t st) {
  if (T == 0) return VCMI_OK;
  if (use_mfma(g)) return dispatch_mfma<1>(g, dX, ldx, T, dLP, g->M, st);
  // no instantiation of the tile kernel (D > 80, or a padded dimension outside its list): tiles streamed through LDS
  if (g->kernel_choice != 1 && g->D > 16 && g->D <= 160) return logdens_tiled_launch(g, dX, ldx, T, dLP, st);
  return gmmmap_generic_launch(g, 1, dX, ldx, T, dLP, g->M, st);
}

int gmmmap_posterior_device(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dP, hipStream_t st) {
  if (T == 0) return VCMI_OK;
  VCMI_TRY(gmmmap_logdens_device(g, dX, ldx, T, dP, st));
  return posterior_finish_launch(0, dP, g->M, T, nullptr, st);
}

int gmmmap_predict_device(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, int64_t *didx, hipStream_t st, bool allow_screen) {
  if (T == 0) return VCMI_OK;
  if (use_mfma(g) && !debug_flag(kDbgPredictTwoPass)) {    // argmax inside the MFMA kernel: no (M,T) matrix, one launch
    // long inputs: frames grouped by nearest source mean, then the screened arg-max (exact; gmmmap_screen.hpp)
    // -- where the model's own frames leave it few survivors (model.argmax_survivors, estimated by profile_model(): 3.7 x on the
    // SURVEY 8d model's frames; on a broad model the bound from four directions never reaches the 40 nats that the full
    // 80-dimensional distance of the best mixture costs, every mixture survives and the early-exit kernel is as fast) and the
    // caller allows it (the trajectory conversion does not: its static + delta vectors are not draws from p(x) -- measured
    // 4.1 against 3.3 ms per 512,000 frames there, tools/predict_screen_ab.py)
    const bool screen_pays = (g->model.argmax_survivors <= kScreenArgmaxFrac || debug_flag(kDbgPredictScreen)) && allow_screen;
    if (screen_pays && g->packedQA.p && g->packedU.p && g->M <= 1024 && can_group(g, T) && !debug_flag(kDbgPredictNoScreen) &&
        !debug_flag(kDbgPredictNoEarlyExit)) {
      int *key = nullptr, *perm = nullptr, *gbase = nullptr;
      VCMI_TRY(launch_grouping(g, dX, ldx, T, st, &key, &perm, &gbase));
      const int rc = dispatch_screen_argmax(g, dX, ldx, T, didx, st, perm, gbase);
      (void)g->grp_order.leave(st);
      return rc;
    }
    // host-prepared handles carry the reversed, tile-by-tile fragments: predict with the exact early exit (MODE 3)
    if (g->packedU2.p && !debug_flag(kDbgPredictNoEarlyExit))
      return dispatch_mfma<3>(g, dX, ldx, T, reinterpret_cast<double *>(didx), 0, st);
    return dispatch_mfma<2>(g, dX, ldx, T, reinterpret_cast<double *>(didx), 0, st);
  }
  StreamOrderScope use(g->grp_order, st);         // (scratch_lp: see gmmmap_convert_device)
  VCMI_TRY(use.status());
  VCMI_TRY(g->scratch_lp.reserve((size_t)T * g->M));
  VCMI_TRY(gmmmap_logdens_device(g, dX, ldx, T, g->scratch_lp.p, st));
  return posterior_finish_launch(1, g->scratch_lp.p, g->M, T, didx, st);
}

}  // namespace vcmi
