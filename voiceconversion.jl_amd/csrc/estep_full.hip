// estep_full.hip -- E-step of EM for a full-covariance GMM on joint features, MI355X (gfx950).
//
// What `gmm[:fit](dataset.X')` does per EM iteration in the reference as shipped
// (bin/train_gmm.jl:84-89 builds sklearn.mixture.GMM(covariance_type="full"); :103 runs EM).  SURVEY 8(f) rank 1.
//   l_nm = log w_m + log N(x_n; mu_m, Sigma_m)   (Cholesky whitening, the fvconvert log-density kernel, MODE 1)
//   gamma = softmax_m(l),  S0_m = sum gamma,  S1_m = sum gamma x,  S2_m = sum gamma x x',  loglik = sum_n lse_n
// Output buffer: [S0 (M) | S1 (Dj,M) | S2 (Dj,Dj,M) | loglik] (one all-reduce).  S2_m is a weighted Gram matrix:
// wave w of an 8-wave workgroup owns mixture 8*mg + w and accumulates the 15 lower 16x16 tiles of its 80x80 S2 with
// v_mfma_f64_16x16x4_f64 (A operand = gamma_f * x_f[i], B operand = x_f[j], k = 4 frames per step); the x tile
// loaded for the A operand is the same register as the B operand of the matching column tile, so a k-step costs
// Dj/16 LDS reads + Dj/16 multiplies for Dj/16*(Dj/16+1)/2 MFMAs.  S0/S1 ride along as per-lane sums of the A operands.
// Per-(mixture group, frame segment) partials are reduced in fixed order -> bit-identical run to run.
#include "estep_internal.hpp"
#include <atomic>
#include "gmmmap_handle.hpp"
#include "hostpipe.hpp"

#include <algorithm>
#include <cmath>

namespace vcmi {

typedef double d4 __attribute__((ext_vector_type(4)));

// log-weighted densities (n,M) -> gamma in place; wave per frame (lanes across mixtures: coalesced rows), fixed grid.
// The per-frame log-sum-exp values are summed per wave in frame order, then per workgroup: lsepart[blockIdx.x].
static constexpr int kSoftmaxGrid = 2048;
__global__ void __launch_bounds__(256)
estep_full_softmax_kernel(double *__restrict__ LP, int M, int64_t n, double *__restrict__ lsepart, unsigned *__restrict__ fmask,
                          int nm) {
  // fmask (optional; mixture groups of nm, at most 32 of them): bit g of fmask[frame] = some mixture of group g has a
  // responsibility that is not exactly zero -- the statistics kernel then visits, per group, only those frames
  __shared__ double wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  if (M <= 32) {
    // Small models (the reference's own: 16 mixtures by default, 32 in its trained ones): 8, 16 or 32 lanes per frame, so a
    // wave takes 8, 4 or 2 frames per turn instead of leaving most of its lanes idle.  The butterflies over lpf lanes give
    // the bits of the 64-lane ones (those only add the zeros of the idle lanes first).
    const int lpf = M <= 8 ? 8 : (M <= 16 ? 16 : 32), fpw = 64 / lpf, sub = lane / lpf, sl = lane % lpf;
    for (int64_t f0 = ((int64_t)blockIdx.x * 4 + wave) * fpw; f0 < n; f0 += (int64_t)gridDim.x * 4 * fpw) {
      const int64_t fr = f0 + sub;
      const bool on = fr < n && sl < M;
      double *l = LP + (fr < n ? fr : n - 1) * M;
      const double lv = on ? l[sl] : -INFINITY;
      double u = lv;
      for (int o = lpf / 2; o >= 1; o >>= 1) u = fmax(u, __shfl_xor(u, o));
      double sm = on ? exp(lv - u) : 0.0;
      for (int o = lpf / 2; o >= 1; o >>= 1) sm += __shfl_xor(sm, o);
      const double ls = u + log(sm);
      unsigned bits = 0;
      if (on) {
        const double gm = exp(lv - ls);
        l[sl] = gm;
        if (gm != 0.0) bits = 1u << ((sl / nm) & 31);
      }
      if (fmask) {
        for (int o = lpf / 2; o >= 1; o >>= 1) bits |= (unsigned)__shfl_xor((int)bits, o);
        if (sl == 0 && fr < n) fmask[fr] = bits;
      }
      if (fr < n) acc += ls;
    }
    // the sub-groups' sums in sub-group order (lanes 0, lpf, 2 lpf, ...)
    double t = 0.0;
    for (int sg = 0; sg < fpw; ++sg) t += __shfl(acc, sg * lpf);
    acc = t;
  } else
  for (int64_t fr = (int64_t)blockIdx.x * 4 + wave; fr < n; fr += (int64_t)gridDim.x * 4) {
    double *l = LP + fr * M;
    double u = -INFINITY;
    for (int m = lane; m < M; m += 64) u = fmax(u, l[m]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) u = fmax(u, __shfl_xor(u, o));
    double sm = 0.0;
    for (int m = lane; m < M; m += 64) sm += exp(l[m] - u);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sm += __shfl_xor(sm, o);
    const double ls = u + log(sm);
    unsigned bits = 0;
    for (int m = lane; m < M; m += 64) {
      const double gm = exp(l[m] - ls);
      l[m] = gm;
      if (gm != 0.0) bits |= 1u << ((m / nm) & 31);
    }
    if (fmask) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) bits |= (unsigned)__shfl_xor((int)bits, o);
      if (lane == 0) fmask[fr] = bits;
    }
    acc += ls;
  }
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) lsepart[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}


// ---- frame lists of the statistics kernel (round 4).  Its workgroup (a mixture group, a frame segment) used to stage EVERY
// frame of its segment -- X travels once per mixture group, 8 x 320 MB through the L2 at M = 64 -- to find that 94 % of the
// 4-frame k-steps carry only exact zeros for its mixtures: the kernel was bound by the fetch / stash / barrier chain of the
// blocks it then skipped.  With fmask (softmax kernel) the frames of a group are listed once -- in frame order: chunk
// histograms, a prefix per group, a stable compaction by ballot / mbcnt, nothing depends on the scheduler -- and the
// statistics kernel walks its group's list.  list[g * n + pos] = frame; total[g] = length.
constexpr int kListChunk = 1024;
__global__ void __launch_bounds__(256)
estep_full_list_count_kernel(const unsigned *__restrict__ fmask, int64_t n, int G, int *__restrict__ chunkcnt) {
  __shared__ int hist[32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 32) hist[tid] = 0;
  __syncthreads();
  const int64_t f0 = (int64_t)blockIdx.x * kListChunk;
  for (int i = 0; i < kListChunk / 256; ++i) {
    const int64_t fr = f0 + 64 * (wave + 4 * i) + lane;
    const unsigned b = fr < n ? fmask[fr] : 0u;
    for (int g = 0; g < G; ++g) {
      const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64((b >> g) & 1u));
      if (lane == 0 && c) atomicAdd(&hist[g], c);
    }
  }
  __syncthreads();
  if (tid < G) chunkcnt[(size_t)blockIdx.x * G + tid] = hist[tid];
}
// one workgroup per group: exclusive prefix of chunkcnt[.][g] over the chunks (in place), total[g]
__global__ void __launch_bounds__(256)
estep_full_list_scan_kernel(int *__restrict__ chunkcnt, int64_t nchunks, int G, int *__restrict__ total) {
  __shared__ int part[256];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int64_t per = (nchunks + 255) / 256, lo = std::min<int64_t>(nchunks, tid * per), hi = std::min<int64_t>(nchunks, lo + per);
  int sum = 0;
  for (int64_t c = lo; c < hi; ++c) sum += chunkcnt[c * G + g];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) {
      const int v = part[i];
      part[i] = run;
      run += v;
    }
    total[g] = run;
  }
  __syncthreads();
  int run = part[tid];
  for (int64_t c = lo; c < hi; ++c) {
    const int v = chunkcnt[c * G + g];
    chunkcnt[c * G + g] = run;
    run += v;
  }
}
__global__ void __launch_bounds__(256)
estep_full_list_fill_kernel(const unsigned *__restrict__ fmask, int64_t n, int G, const int *__restrict__ chunkoff,
                            int *__restrict__ list) {
  __shared__ int rowcnt[16][32];           // frames of group g in row r of the chunk -> exclusive prefix over the rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t f0 = (int64_t)blockIdx.x * kListChunk;
  unsigned b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = wave + 4 * i;
    const int64_t fr = f0 + 64 * r + lane;
    b[i] = fr < n ? fmask[fr] : 0u;
    for (int g = 0; g < G; ++g) {
      const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64((b[i] >> g) & 1u));
      if (lane == 0) rowcnt[r][g] = c;
    }
  }
  __syncthreads();
  if (tid < G) {
    int run = 0;
    for (int r = 0; r < 16; ++r) {
      const int v = rowcnt[r][tid];
      rowcnt[r][tid] = run;
      run += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = wave + 4 * i;
    const int64_t fr = f0 + 64 * r + lane;
    for (int g = 0; g < G; ++g) {
      const unsigned long long mask = __builtin_amdgcn_ballot_w64((b[i] >> g) & 1u);
      if ((b[i] >> g) & 1u) {
        const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
        list[(size_t)g * n + chunkoff[(size_t)blockIdx.x * G + g] + rowcnt[r][g] + below] = (int)fr;
      }
    }
  }
}

static constexpr int kFullFB = 32;   // frames per staged block (double-buffered in LDS)

// lower tiles of a (16 NTL)^2 symmetric matrix in row-major order: tile t -> (row tile a, column tile j <= a)
__host__ __device__ constexpr int full_tile_a(int t) {
  int a = 0;
  while ((a + 1) * (a + 2) / 2 <= t) ++a;
  return a;
}
__host__ __device__ constexpr int full_tile_j(int t) { return t - full_tile_a(t) * (full_tile_a(t) + 1) / 2; }

// the tiles [T0, T0 + NTP) as compile-time tables: row / column tile of each, and which x tiles they read as rows / columns
template <int T0, int NTP>
struct FullTileList {
  int a[NTP > 0 ? NTP : 1], j[NTP > 0 ? NTP : 1];
  unsigned rows, cols;
  constexpr FullTileList() : a{}, j{}, rows(0), cols(0) {
    for (int t = 0; t < NTP; ++t) {
      a[t] = full_tile_a(T0 + t);
      j[t] = full_tile_j(T0 + t);
      rows |= 1u << a[t];
      cols |= 1u << j[t];
    }
  }
};

template <int DJ, int PARTS>
struct FullStatsCfg {
  static constexpr int NTL = DJ / 16, NTILES = NTL * (NTL + 1) / 2;
  static constexpr int TPP = (NTILES + PARTS - 1) / PARTS;     // tiles per part (consecutive tiles: few distinct operands)
  static constexpr int NM = 8 / PARTS;                          // mixtures per workgroup
  // row stride == 16 (mod 32) doubles: the four 16-lane groups of an operand read (4 consecutive frames) then fall in
  // disjoint halves of the 64 LDS banks per half-wave
  static constexpr int RSX = (DJ % 32 == 16) ? DJ : DJ + 16;
  static constexpr size_t LDS_BYTES = ((size_t)2 * kFullFB * RSX + 2 * kFullFB * 8) * sizeof(double);
};

// The body of one wave: mixture `m`, tiles [PART TPP, (PART+1) TPP) of its S2 (and, for the last part, S0 and S1).
// Wave w of an 8-wave workgroup owns mixture NM mg + w / PARTS and part w % PARTS: at DJ = 80 one wave holds all 15 lower
// tiles of its mixture (PARTS = 1); at DJ = 160 the 55 tiles (220 accumulator registers) are shared by four waves.
template <int DJ, int PARTS, int PART>
__device__ __forceinline__ void estep_full_stats_body(const double *__restrict__ X, int64_t n0, int64_t f_begin, int64_t f_end,
                                                      int M, int mg, const double *__restrict__ G, double *__restrict__ P,
                                                      double *xs, double *gs, int dj, const int *__restrict__ lst,
                                                      unsigned long long *__restrict__ mfma_count) {
  // lst (optional): positions [f_begin, f_end) index this mixture group's frame list instead of the frames themselves
  using C = FullStatsCfg<DJ, PARTS>;
  constexpr int NTL = C::NTL, RSX = C::RSX, FB = kFullFB, NM = C::NM;
  constexpr int T0 = PART * C::TPP, T1 = (T0 + C::TPP < C::NTILES) ? T0 + C::TPP : C::NTILES, NTP = T1 - T0;
  constexpr bool kFirstMoments = PART == PARTS - 1;        // the last part has the fewest tiles: it also sums S0 and S1
  constexpr int NPF = (FB * DJ + 511) / 512;               // staged doubles per thread per block
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lcol = lane & 15, lgrp = lane >> 4;
  const int ml = wave / PARTS, m = mg * NM + ml;           // this wave's mixture (may be >= M: then gamma is staged as 0)

  d4 acc[NTP > 0 ? NTP : 1];
#pragma unroll
  for (int t = 0; t < NTP; ++t) acc[t] = d4{0, 0, 0, 0};
  double s1[NTL], s0 = 0.0;
#pragma unroll
  for (int a = 0; a < NTL; ++a) s1[a] = 0.0;
  int nmfma = 0;               // MFMAs this wave issued (measurement: mfma_count, optional)

  double pf[NPF], pg = 0.0;
  const int gf = tid / NM, gq = tid % NM;                 // gamma staging: FB frames x NM mixtures
  const int gm_idx = mg * NM + gq;
  // element i of this thread: row (frame of the block) and column of the staged image (dj <= DJ is the data's dimension;
  // the columns dj .. DJ-1 of the LDS image are never written: they only reach accumulators that are not stored)
  int rowi[NPF], coli[NPF];
#pragma unroll
  for (int i = 0; i < NPF; ++i) {
    const int e = tid + 512 * i;
    rowi[i] = e / dj;
    coli[i] = e - rowi[i] * dj;
  }
  // the frames of the block that is fetched NEXT (list mode: read one block ahead of the rows they address)
  int fidx[NPF], gfidx = 0;                               // (a call's chunk has at most 2^20 frames)
  auto load_idx = [&](int64_t fb) {
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      const int64_t pos = fb + rowi[i];
      fidx[i] = (lst && rowi[i] < FB && pos < f_end) ? lst[pos] : (int)pos;
    }
    gfidx = (lst && tid < FB * NM && fb + gf < f_end) ? lst[fb + gf] : (int)(fb + gf);
  };
  auto fetch = [&](int64_t fb) {                           // global -> registers
#pragma unroll
    for (int i = 0; i < NPF; ++i)
      pf[i] = (rowi[i] < FB && fb + rowi[i] < f_end) ? X[(n0 + (int64_t)fidx[i]) * dj + coli[i]] : 0.0;
    pg = (tid < FB * NM && fb + gf < f_end && gm_idx < M) ? G[(int64_t)gfidx * M + gm_idx] : 0.0;
  };
  auto stash = [&](int buf) {                              // registers -> LDS
#pragma unroll
    for (int i = 0; i < NPF; ++i)
      if (rowi[i] < FB) xs[buf * FB * RSX + rowi[i] * RSX + coli[i]] = pf[i];
    if (tid < FB * NM) gs[buf * FB * 8 + gf * NM + gq] = pg;
  };
  constexpr FullTileList<T0, NTP> TL{};                   // which x tiles this part reads, which of them it scales by gamma

  if (dj < DJ) {                                          // padding columns: finite values (they are multiplied, never stored)
    for (int e = tid; e < 2 * FB * RSX; e += 512) xs[e] = 0.0;
    __syncthreads();
  }
  if (f_begin < f_end) {
    load_idx(f_begin);
    fetch(f_begin);
    stash(0);
    load_idx(f_begin + FB);
  }
  __syncthreads();
  int buf = 0;
  for (int64_t fb = f_begin; fb < f_end; fb += FB, buf ^= 1) {
    const bool more = fb + FB < f_end;
    if (more) {
      fetch(fb + FB);
      load_idx(fb + 2 * FB);
    }
    const double *xb = xs + buf * FB * RSX, *gb = gs + buf * FB * 8;
#pragma unroll 2
    for (int ks = 0; ks < FB / 4; ++ks) {
      const int f = 4 * ks + lgrp;
      const double gm = gb[f * NM + ml];
      // the four frames of the k-step all have gamma == 0 exactly for this wave's mixture (l_m more than 745 nats under
      // the frame's maximum): the products add exactly nothing -- skipped (wave-uniform; bit-identical statistics)
      if (__builtin_amdgcn_ballot_w64(gm != 0.0) == 0) continue;
      nmfma += NTP;
      const double *xr = xb + f * RSX + lcol;
      double xv[NTL], ax[NTL];
#pragma unroll
      for (int a = 0; a < NTL; ++a) {
        if (kFirstMoments || (((TL.rows | TL.cols) >> a) & 1u)) xv[a] = xr[16 * a];
        if (kFirstMoments || ((TL.rows >> a) & 1u)) ax[a] = gm * xv[a];
        if (kFirstMoments) s1[a] += ax[a];
      }
      if (kFirstMoments) s0 += gm;
#pragma unroll
      for (int t = 0; t < NTP; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ax[TL.a[t]], xv[TL.j[t]], acc[t], 0, 0, 0);
    }
    if (more) stash(buf ^ 1);
    __syncthreads();
  }
  if (mfma_count && lane == 0) atomicAdd(mfma_count, (unsigned long long)nmfma);
  if (m >= M) return;
  // partial statistics of this (mixture, segment) in the final layout [S0 | S1 | S2 | loglik]
  if (kFirstMoments) {
    s0 += __shfl_xor(s0, 16);
    s0 += __shfl_xor(s0, 32);
    if (lane == 0) P[m] = s0;
#pragma unroll
    for (int a = 0; a < NTL; ++a) {
      double v = s1[a];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (lgrp == 0 && 16 * a + lcol < dj) P[M + (size_t)m * dj + 16 * a + lcol] = v;
    }
  }
  double *S2 = P + M + (size_t)M * dj + (size_t)m * dj * dj;      // (dj,dj) column-major
#pragma unroll
  for (int t = 0; t < NTP; ++t) {
    const int a = TL.a[t], j = TL.j[t];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * a + lgrp + 4 * r, jc = 16 * j + lcol;    // D[i][jc]
      if ((a != j || i >= jc) && i < dj && jc < dj) {              // diagonal tiles: lower part only, then mirrored
        S2[i + (size_t)dj * jc] = acc[t][r];
        S2[jc + (size_t)dj * i] = acc[t][r];
      }
    }
  }
}

template <int DJ, int PARTS>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
estep_full_stats_kernel(const double *__restrict__ X, int64_t n0, int64_t n, int M, const double *__restrict__ G,
                        double *__restrict__ part, int64_t plen, int dj, const int *__restrict__ lists,
                        const int *__restrict__ totals, unsigned long long *__restrict__ mfma_count) {
  static_assert(DJ % 16 == 0, "full-covariance MFMA statistics need Dj to be a multiple of 16");
  static_assert(PARTS == 1 || PARTS == 2 || PARTS == 4, "waves per mixture");
  using C = FullStatsCfg<DJ, PARTS>;
  extern __shared__ double fsm[];
  double *xs = fsm;                                     // [2][FB][RSX]
  double *gs = fsm + 2 * kFullFB * C::RSX;              // [2][FB][8]
  // grid = (frame segments, mixture groups): consecutive workgroups go to consecutive XCDs, so with the segment as the
  // FAST index the mixture groups that read one segment of X share an XCD (when the segment count is a multiple of 8)
  // and X reaches that L2 once instead of once per mixture group
  const int mg = blockIdx.y, seg = blockIdx.x, nsegs = gridDim.x;
  // with frame lists the segment is a range of POSITIONS in this mixture group's list (its length is on the device)
  const int64_t len = lists ? (int64_t)totals[mg] : n;
  const int *lst = lists ? lists + (size_t)mg * n : nullptr;
  const int64_t seglen = (len + nsegs - 1) / nsegs;
  const int64_t f_begin = std::min<int64_t>(len, seg * seglen), f_end = (f_begin + seglen < len) ? f_begin + seglen : len;
  double *P = part + (size_t)seg * plen;
  const int prt = (threadIdx.x >> 6) % PARTS;          // wave-uniform; every branch runs the same number of barriers
  if (PARTS == 1 || prt == 0) estep_full_stats_body<DJ, PARTS, 0>(X, n0, f_begin, f_end, M, mg, G, P, xs, gs, dj, lst, mfma_count);
  else if (PARTS == 2 || prt == 1) estep_full_stats_body<DJ, PARTS, 1>(X, n0, f_begin, f_end, M, mg, G, P, xs, gs, dj, lst, mfma_count);
  else if (prt == 2) estep_full_stats_body<DJ, PARTS, (PARTS > 2 ? 2 : 0)>(X, n0, f_begin, f_end, M, mg, G, P, xs, gs, dj, lst, mfma_count);
  else estep_full_stats_body<DJ, PARTS, (PARTS > 3 ? 3 : 0)>(X, n0, f_begin, f_end, M, mg, G, P, xs, gs, dj, lst, mfma_count);
}

// generic statistics (any Dj): thread per lower-triangle element of one mixture's S2 (+ S1, S0), sequential over the
// frames of one segment
__global__ void __launch_bounds__(256)
estep_full_stats_generic_kernel(const double *__restrict__ X, int64_t n0, int64_t n, int Dj, int M,
                                const double *__restrict__ G, double *__restrict__ part, int64_t plen) {
  const int m = blockIdx.x;
  const int64_t seglen = (n + gridDim.y - 1) / gridDim.y;
  const int64_t f_begin = blockIdx.y * seglen, f_end = (f_begin + seglen < n) ? f_begin + seglen : n;
  double *P = part + (size_t)blockIdx.y * plen;
  double *S2 = P + M + (size_t)M * Dj + (size_t)m * Dj * Dj;
  const int ntri = Dj * (Dj + 1) / 2;
  for (int e = threadIdx.x; e < ntri + Dj + 1; e += 256) {
    double s = 0.0;
    if (e < ntri) {
      int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) / 2.0);
      while (i * (i + 1) / 2 > e) --i;
      while ((i + 1) * (i + 2) / 2 <= e) ++i;
      const int j = e - i * (i + 1) / 2;
      for (int64_t f = f_begin; f < f_end; ++f) s = fma(G[f * M + m] * X[(n0 + f) * Dj + i], X[(n0 + f) * Dj + j], s);
      S2[i + (size_t)Dj * j] = s;
      S2[j + (size_t)Dj * i] = s;
    } else if (e < ntri + Dj) {
      const int d = e - ntri;
      for (int64_t f = f_begin; f < f_end; ++f) s = fma(G[f * M + m], X[(n0 + f) * Dj + d], s);
      P[M + (size_t)m * Dj + d] = s;
    } else {
      for (int64_t f = f_begin; f < f_end; ++f) s += G[f * M + m];
      P[m] = s;
    }
  }
}

struct EstepFullScratch {
  DevBuf<double> LP, lse, part, params;
  DevBuf<int> flag;
  DevBuf<unsigned long long> mfma_count;   // optional measurement counter of the statistics kernel (vcmi_debug_estep_full_mfma)
  DevBuf<int> lists;        // frame lists of the statistics kernel: [fmask (n) | chunk counts (nchunks, G) | totals (G) | lists (G, n)]
  vcmi_gmmmap *px = nullptr;
  StreamOrder order;   // calls of one thread on different streams share the buffers above
  ~EstepFullScratch() { delete px; }
};
static EstepFullScratch &full_scratch() {
  static thread_local EstepFullScratch s;
  return s;
}

// statistics of N device-resident frames under the prepared p(x) handle -> dstats (zeroed here); asynchronous on st, inside the
// caller's StreamOrderScope
static int estep_full_stats(EstepFullScratch &sc, vcmi_gmmmap *px, const double *dX, int64_t N, int Dj, int M, double *dstats,
                            hipStream_t st) {
  const int64_t plen = (int64_t)M * (1 + Dj + (int64_t)Dj * Dj) + 1;
  VCMI_HIP(hipMemsetAsync(dstats, 0, plen * sizeof(double), st));
  if (N == 0) return VCMI_OK;
  const int64_t chunk = std::min<int64_t>(N, (int64_t)1 << 20);
  VCMI_TRY(sc.LP.reserve((size_t)chunk * M));
  VCMI_TRY(sc.lse.reserve((size_t)kSoftmaxGrid));
  // frame segments (grid.x): one 8-wave workgroup per CU in a single round, whatever the mixture count; a workgroup
  // holds 8 mixtures up to Dj = 80 and 2 (four waves per mixture) beyond
  // MFMA statistics for every Dj <= 160, in the smallest of the instantiations 32, 48, 64, 80 (one wave per mixture) and
  // 96, 128, 160 (four) that holds it
  const bool mfma = Dj <= 160 && !debug_flag(kDbgEstepGeneric);
  const int nm = (!mfma || Dj <= 80) ? 8 : 2;
  const int mgroups = (M + nm - 1) / nm;
  const int nseg = std::max(1, (256 + mgroups - 1) / mgroups);
  VCMI_TRY(sc.part.reserve((size_t)nseg * plen));
  for (int64_t n0 = 0; n0 < N; n0 += chunk) {
    const int64_t n = std::min<int64_t>(chunk, N - n0);
    VCMI_TRY(gmmmap_logdens_device(px, dX + n0 * Dj, Dj, n, sc.LP.p, st));
    // frame lists per mixture group (MFMA statistics, at most 32 groups, enough frames to matter)
    const bool use_lists = mfma && mgroups <= 32 && n >= 4096 && !debug_flag(kDbgEstepFullNoLists);
    unsigned *fmask = nullptr;
    int *chunkcnt = nullptr, *totals = nullptr, *lists = nullptr;
    const int64_t nlc = (n + kListChunk - 1) / kListChunk;
    if (use_lists) {
      VCMI_TRY(sc.lists.reserve((size_t)n + (size_t)nlc * mgroups + mgroups + (size_t)mgroups * n));
      fmask = reinterpret_cast<unsigned *>(sc.lists.p);
      chunkcnt = sc.lists.p + n;
      totals = chunkcnt + (size_t)nlc * mgroups;
      lists = totals + mgroups;
    }
    hipLaunchKernelGGL(estep_full_softmax_kernel, dim3(kSoftmaxGrid), dim3(256), 0, st, sc.LP.p, M, n, sc.lse.p, fmask, nm);
    estep_sum_launch(sc.lse.p, (int64_t)kSoftmaxGrid, dstats + (plen - 1), st);
    if (use_lists) {
      hipLaunchKernelGGL(estep_full_list_count_kernel, dim3((unsigned)nlc), dim3(256), 0, st, fmask, n, mgroups, chunkcnt);
      hipLaunchKernelGGL(estep_full_list_scan_kernel, dim3((unsigned)mgroups), dim3(256), 0, st, chunkcnt, nlc, mgroups, totals);
      hipLaunchKernelGGL(estep_full_list_fill_kernel, dim3((unsigned)nlc), dim3(256), 0, st, fmask, n, mgroups, chunkcnt, lists);
    }
    VCMI_HIP(hipMemsetAsync(sc.part.p, 0, (size_t)nseg * plen * sizeof(double), st));
    const dim3 grid(nseg, mgroups);
    if (mfma) {
      auto launch = [&](auto kern, size_t lds) -> int {
        static std::atomic<bool> attr_done[64];           // per instantiation (the lambda is generic) and per device
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (!attr_done[dev & 63].load(std::memory_order_acquire)) {
          VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
          attr_done[dev & 63].store(true, std::memory_order_release);
        }
        hipLaunchKernelGGL(kern, grid, dim3(512), lds, st, dX, n0, n, M, sc.LP.p, sc.part.p, plen, Dj, (const int *)lists,
                           (const int *)totals, sc.mfma_count.p);
        return VCMI_OK;
      };
      if (Dj <= 32) VCMI_TRY(launch(estep_full_stats_kernel<32, 1>, FullStatsCfg<32, 1>::LDS_BYTES));
      else if (Dj <= 48) VCMI_TRY(launch(estep_full_stats_kernel<48, 1>, FullStatsCfg<48, 1>::LDS_BYTES));
      else if (Dj <= 64) VCMI_TRY(launch(estep_full_stats_kernel<64, 1>, FullStatsCfg<64, 1>::LDS_BYTES));
      else if (Dj <= 80) VCMI_TRY(launch(estep_full_stats_kernel<80, 1>, FullStatsCfg<80, 1>::LDS_BYTES));
      else if (Dj <= 96) VCMI_TRY(launch(estep_full_stats_kernel<96, 4>, FullStatsCfg<96, 4>::LDS_BYTES));
      else if (Dj <= 128) VCMI_TRY(launch(estep_full_stats_kernel<128, 4>, FullStatsCfg<128, 4>::LDS_BYTES));
      else VCMI_TRY(launch(estep_full_stats_kernel<160, 4>, FullStatsCfg<160, 4>::LDS_BYTES));
    } else {
      hipLaunchKernelGGL(estep_full_stats_generic_kernel, dim3(M, nseg), dim3(256), 0, st, dX, n0, n, Dj, M, sc.LP.p,
                         sc.part.p, plen);
    }
    // the loglik slot of the partial rows is zero, so the generic reduction leaves dstats[plen-1] (set above) intact
    estep_reduce_launch(sc.part.p, nseg, plen, dstats, st);
    VCMI_HIP(hipGetLastError());
  }
  return VCMI_OK;
}

int estep_full_core(vcmi_gmmmap *px, const double *dX, int64_t N, int Dj, int M, double *dstats, hipStream_t st) {
  EstepFullScratch &sc = full_scratch();
  StreamOrderScope use(sc.order, st);
  VCMI_TRY(use.status());
  return estep_full_stats(sc, px, dX, N, Dj, M, dstats, st);
}

int read_pd_flag(const int *d_flag, hipStream_t st) {
  int h = 0;
  VCMI_HIP(hipMemcpyAsync(&h, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  VCMI_HIP(hipStreamSynchronize(st));
  if (h) return fail(VCMI_ERR_NOT_PD, "covariance of mixture %d is not positive definite", h);
  return VCMI_OK;
}

// one E-step from HOST parameters: upload (Dj*Dj*M doubles), Cholesky whitening of every mixture on the device
// (px_prep_kernel; host fallback for very large Dj), statistics, then the stream is drained (the p(x) handle and the
// parameter staging buffers persist per host thread and are rewritten by the next call).
static int estep_full_device(const double *dX, int64_t N, int Dj, int M, const double *w, const double *mu,
                             const double *sigma, double *dstats, hipStream_t st) {
  VCMI_TRY(estep_check_dims(N, Dj, M));
  if (!w || !mu || !sigma || !dstats || (N > 0 && !dX)) return fail(VCMI_ERR_ARG, "E-step: NULL argument");
  EstepFullScratch &sc = full_scratch();
  const bool on_device = gmm_px_device_prepare_supported(Dj);
  {   // the parameter staging and the p(x) handle are rewritten before the statistics run; the host waits outside the scope
    StreamOrderScope use(sc.order, st);
    VCMI_TRY(use.status());
    if (N == 0) return estep_full_stats(sc, nullptr, dX, 0, Dj, M, dstats, st);
    if (on_device) {
      const size_t dd = (size_t)Dj * Dj;
      VCMI_TRY(sc.params.reserve((size_t)M * (1 + Dj + dd)));
      VCMI_TRY(sc.flag.reserve(1));
      double *dw = sc.params.p, *dmu = dw + M, *dsig = dmu + (size_t)M * Dj;
      VCMI_TRY(staged_upload(dw, w, sizeof(double) * M, st));      // (through the pinned ring: hostpipe.hpp, upload_now)
      VCMI_TRY(staged_upload(dmu, mu, sizeof(double) * M * Dj, st));      // (through the pinned ring: hostpipe.hpp, upload_now)
      VCMI_TRY(staged_upload(dsig, sigma, sizeof(double) * M * dd, st));      // (through the pinned ring: hostpipe.hpp, upload_now)
      VCMI_HIP(hipMemsetAsync(sc.flag.p, 0, sizeof(int), st));
      VCMI_TRY(gmm_px_prepare_device(&sc.px, dw, dmu, dsig, Dj, M, sc.flag.p, st));
    } else {
      VCMI_TRY(gmm_px_create(w, mu, sigma, Dj, M, &sc.px));
    }
    VCMI_TRY(estep_full_stats(sc, sc.px, dX, N, Dj, M, dstats, st));
  }
  if (on_device) return read_pd_flag(sc.flag.p, st);
  VCMI_HIP(hipStreamSynchronize(st));
  return VCMI_OK;
}

}  // namespace vcmi

using namespace vcmi;

extern "C" int64_t vcmi_estep_full_stats_len(int Dj, int M) { return (int64_t)M * (1 + Dj + (int64_t)Dj * Dj) + 1; }

extern "C" int vcmi_estep_full_dev(const double *dX, int64_t N, int Dj, int M, const double *w, const double *mu,
                                   const double *sigma, double *dstats, void *stream) {
  return estep_full_device(dX, N, Dj, M, w, mu, sigma, dstats, as_stream(stream));
}

extern "C" int vcmi_estep_full(const double *X, int64_t N, int Dj, int M, const double *w, const double *mu,
                               const double *sigma, double *S0, double *S1, double *S2, double *loglik) {
  if (!S0 || !S1 || !S2 || !loglik) return fail(VCMI_ERR_ARG, "vcmi_estep_full: NULL output");
  VCMI_TRY(estep_check_dims(N, Dj, M));
  if (N > 0 && !X) return fail(VCMI_ERR_ARG, "vcmi_estep_full: NULL frames");
  return estep_host(estep_full_device, X, N, Dj, M, w, mu, sigma, vcmi_estep_full_stats_len(Dj, M), (size_t)M * Dj * Dj, S0, S1, S2,
                    loglik);
}

// Measurement hook (not part of include/vcmi.h), as vcmi_debug_estep_mfma: the MFMAs of the full-covariance STATISTICS kernel
// (its log-density kernel issues a fixed, known number of them).
extern "C" int vcmi_debug_estep_full_mfma(int enable, int64_t *issued) { return mfma_count_hook(full_scratch().mfma_count, enable, issued); }
