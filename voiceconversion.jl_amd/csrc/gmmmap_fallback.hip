// gmmmap_fallback.hip -- fvconvert, log-densities, posterior and argmax for the dimensions and settings the tile kernel of
// gmmmap.hip does not serve: the generic FP64 VALU kernel (any D), the tiled MFMA log-densities for padded dimensions
// without a tile instantiation up to 160 with the conversion that follows them, and the finish of an (M,T) log-density
// matrix.  gmmmap.hip decides which of them runs; the host launch functions at the end are declared in gmmmap_fallback.hpp.
#include "gmmmap_fallback.hpp"
#include "gmmmap_handle.hpp"
#include "fp64_exp.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <type_traits>

namespace vcmi {

// ------------------------------------------------------------------------------------------------
// Generic VALU kernel (any D): one lane per frame, x and the y accumulator in LDS ([d][lane] layout,
// conflict-free), parameters read through wave-uniform (scalar) loads.
// MODE 0 convert, 1 log-weighted densities (M,T).
// ------------------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(64)
gmmmap_generic_kernel(const double *__restrict__ U, const double *__restrict__ A, const double *__restrict__ cz,
                      const double *__restrict__ b, const double *__restrict__ lcv, int M, int D, int DP,
                      const double *__restrict__ X, int64_t ldx, int64_t T, double *__restrict__ Y, int64_t ldy) {
  extern __shared__ double smem[];
  double *xs = smem;              // [D][64]
  double *ys = smem + (size_t)D * 64;   // [D][64] (MODE 0)
  const int lane = threadIdx.x;
  const int64_t fr = (int64_t)blockIdx.x * 64 + lane;
  const bool live = fr < T;
  for (int d = 0; d < D; ++d) {
    xs[d * 64 + lane] = live ? X[fr * ldx + d] : 0.0;
    if (MODE == 0) ys[d * 64 + lane] = 0.0;
  }
  double runmax = -INFINITY, den = 0.0;
  for (int m = 0; m < M; ++m) {
    const double lc = lcv[m];
    if (lc == -INFINITY) {
      if (MODE == 1 && live) Y[fr * ldy + m] = -INFINITY;
      continue;
    }
    const double *Um = U + (size_t)m * DP * DP;
    double q = 0.0;
    for (int i = 0; i < D; ++i) {
      double z = -cz[(size_t)m * DP + i];
      for (int j = 0; j <= i; ++j) z = fma(Um[i * DP + j], xs[j * 64 + lane], z);
      q = fma(z, z, q);
    }
    const double l = lc - 0.5 * q;
    if (MODE == 1) {
      if (live) Y[fr * ldy + m] = l;
    } else {
      const double nm = fmax(runmax, l);
      const double sc = vc_exp(runmax - nm);
      const double wg = vc_exp(l - nm);
      den = fma(den, sc, wg);
      runmax = nm;
      const double *Am = A + (size_t)m * DP * DP;
      for (int i = 0; i < D; ++i) {
        double e = b[(size_t)m * DP + i];
        for (int j = 0; j < D; ++j) e = fma(Am[i * DP + j], xs[j * 64 + lane], e);
        ys[i * 64 + lane] = fma(wg, e, ys[i * 64 + lane] * sc);
      }
    }
  }
  if (MODE == 0 && live) {
    const double inv = 1.0 / den;
    for (int d = 0; d < D; ++d) Y[fr * ldy + d] = ys[d * 64 + lane] * inv;
  }
}

// ------------------------------------------------------------------------------------------------
// Log-weighted densities for the dimensions the MFMA kernel above is not instantiated for, up to D = 16 NTMAX -- above all
// 80 < D <= 160 (e.g. the 160-dimensional joint GMM of delta-augmented features that TrajectoryGMMMap is trained from):
// the x operands of that kernel (D/4 k-steps x FT tiles) and a mixture's whitening block (103 KB at D = 160) no longer
// fit registers / a double-buffered LDS block, so here
//   * a workgroup owns 128 frames: wave w keeps the B-operand fragments of its 16 frames (D/4 doubles per lane) for the
//     whole kernel;
//   * the whitening blocks stream through LDS one 16-row tile at a time ("piece": rows 16r .. 16r+15, the 16(r+1)
//     columns up to the diagonal, straight from the row-major U of the generic layout, zeros above the diagonal),
//     double-buffered: the next piece travels global -> registers during the products of the current one;
//   * z = U x - cz per row tile: accumulators start from -cz, 4(r+1) v_mfma_f64_16x16x4 per tile and wave, |z|^2 summed
//     per frame across the row tiles and the four lane groups.
// Row stride of a piece == 18 (mod 32) doubles: the 16-row fragment reads are conflict-free (as in estep.hip).
// ------------------------------------------------------------------------------------------------
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &f) {     // f(integral_constant<int, I>) for I .. N-1, unrolled at compile time
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// Stages of a mixture's whitening block: consecutive row tiles staged and multiplied together.  The first row tiles are
// short (4, 8, 12 ... k-steps): taken one at a time their products do not cover the latency of the next piece's loads,
// so the stages are cut to at least ~28 k-steps each (at NTMAX = 10: tiles 0-3 | 4-5 | 6 | 7 | 8 | 9).
template <int NTMAX>
struct TiledStages {
  static constexpr int kMinSteps = 28;
  int first[NTMAX], last[NTMAX], n;
  constexpr TiledStages() : first{}, last{}, n(0) {
    int r = 0;
    while (r < NTMAX) {
      int e = r, steps = 4 * (r + 1);
      while (steps < kMinSteps && e + 1 < NTMAX) {
        ++e;
        steps += 4 * (e + 1);
      }
      first[n] = r;
      last[n] = e;
      ++n;
      r = e + 1;
    }
  }
  constexpr int rows(int s) const { return 16 * (last[s] - first[s] + 1); }
  constexpr int cols(int s) const { return 16 * (last[s] + 1); }
  constexpr int rs(int s) const { return (cols(s) + 13) / 32 * 32 + 18; }        // == 18 (mod 32): conflict-free fragment reads
  constexpr int piece(int s) const { return rows(s) * rs(s) + rows(s); }         // + the rows' cz values
  constexpr int max_piece() const {
    int v = 0;
    for (int s = 0; s < n; ++s) v = piece(s) > v ? piece(s) : v;
    return v;
  }
};

template <int NTMAX>
__global__ void __launch_bounds__(512)
logdens_tiled_kernel(const double *__restrict__ U, const double *__restrict__ cz, const double *__restrict__ lcv, int M, int D,
                     int DP, const double *__restrict__ X, int64_t ldx, int64_t T, double *__restrict__ LP, int64_t ldy) {
  constexpr int KSMAX = 4 * NTMAX;
  constexpr TiledStages<NTMAX> ST{};
  constexpr int PIECE = ST.max_piece();
  constexpr int NPRE = 4;                               // staged pairs per thread: 512 x 4 x 2 doubles >= the largest stage
  extern __shared__ double tsm[];                       // [2][PIECE]
  typedef double d2 __attribute__((ext_vector_type(2)));
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lcol = lane & 15, lgrp = lane >> 4;
  const int NT = (D + 15) / 16;
  const int64_t f = (int64_t)blockIdx.x * 128 + 16 * wave + lcol;
  const int64_t fc = f < T ? f : T - 1;               // frames beyond T read a valid row and are not written

  double xfrag[KSMAX];
#pragma unroll
  for (int ks = 0; ks < KSMAX; ++ks) {
    const int k = 4 * ks + lgrp;
    xfrag[ks] = (k < D) ? X[fc * ldx + k] : 0.0;
  }

  // staging of stage s of mixture m: element pairs (row, 2 c2) of the rows x cols block, zeros above the diagonal and
  // beyond D
  d2 pre[NPRE];
  double precz = 0.0;
  auto fetch = [&](int m, auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr int W2 = ST.cols(s) / 2, NP = (ST.rows(s) * W2 + 511) / 512, R0 = 16 * ST.first[s];
    static_assert(NP <= NPRE, "stage larger than the staging registers");
    const double *Um = U + (size_t)m * DP * DP;
    // every load is unconditional on a clamped address (a branch or a select on the loaded value would make the wave
    // wait for each load in turn); the zeros above the diagonal and beyond D are applied when the values go to LDS
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int e0 = tid + 512 * i, e = e0 < ST.rows(s) * W2 ? e0 : 0;
      const int row = e / W2, c = 2 * (e - row * W2), gr = R0 + row;
      const int grc = gr < D ? gr : D - 1, cc = c + 1 < DP ? c : DP - 2;
      pre[i] = *reinterpret_cast<const d2 *>(Um + (size_t)grc * DP + cc);
    }
    const int zr = (tid < ST.rows(s) && R0 + tid < D) ? R0 + tid : 0;
    precz = cz[(size_t)m * DP + zr];
  };
  auto stash = [&](double *dst, auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr int W2 = ST.cols(s) / 2, NP = (ST.rows(s) * W2 + 511) / 512, RS = ST.rs(s);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int e = tid + 512 * i;
      if (e < ST.rows(s) * W2) {
        const int row = e / W2, c = 2 * (e - row * W2), gr = 16 * ST.first[s] + row;
        d2 v = pre[i];
        v.x = (gr < D && c <= gr) ? v.x : 0.0;
        v.y = (gr < D && c + 1 <= gr) ? v.y : 0.0;
        *reinterpret_cast<d2 *>(dst + row * RS + c) = v;
      }
    }
    if (tid < ST.rows(s)) dst[ST.rows(s) * RS + tid] = (16 * ST.first[s] + tid < D) ? precz : 0.0;
  };
  // one stage: the next one -- (m, s+1), or (m+1, 0) -- travels global -> registers during the products, registers -> the
  // other LDS buffer after them
  auto step = [&](int m, auto sc, double *cur, double *nxt, double &q) {
    constexpr int s = decltype(sc)::value;
    constexpr int RS = ST.rs(s), SN = (s + 1 < ST.n) ? s + 1 : 0;
    const bool more_here = (s + 1 < ST.n) && (ST.first[SN] < NT);
    if (more_here) fetch(m, std::integral_constant<int, SN>{});
    else if (m + 1 < M) fetch(m + 1, std::integral_constant<int, 0>{});
#pragma unroll
    for (int r = ST.first[s]; r <= ST.last[s]; ++r) {
      if (r < NT) {                                     // workgroup-uniform
        const int lr = 16 * (r - ST.first[s]);
        // two accumulator chains (even / odd k-steps), the A fragments read four k-steps ahead of their products
        d4 acc, acc2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = -cur[ST.rows(s) * RS + lr + 4 * i + lgrp];
        const double *ap = cur + (lr + lcol) * RS + lgrp;
        constexpr int NK = 4, AHEAD = 4;
        const int nks = NK * (r + 1);
        double af[AHEAD];
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) af[i] = ap[4 * i];
#pragma unroll
        for (int ks = 0; ks < nks; ks += AHEAD) {
          double an[AHEAD];
#pragma unroll
          for (int i = 0; i < AHEAD; ++i) an[i] = (ks + AHEAD + i < nks) ? ap[4 * (ks + AHEAD + i)] : 0.0;
#pragma unroll
          for (int i = 0; i < AHEAD; i += 2) {
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], xfrag[ks + i], acc, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i + 1], xfrag[ks + i + 1], acc2, 0, 0, 0);
          }
#pragma unroll
          for (int i = 0; i < AHEAD; ++i) af[i] = an[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double z = acc[i] + acc2[i];
          q = fma(z, z, q);
        }
      }
    }
    if (more_here) stash(nxt, std::integral_constant<int, SN>{});
    else if (m + 1 < M) stash(nxt, std::integral_constant<int, 0>{});
    __syncthreads();
  };

  fetch(0, std::integral_constant<int, 0>{});
  stash(tsm, std::integral_constant<int, 0>{});
  __syncthreads();
  int pc = 0;                                           // stages done: buffer parity
  for (int m = 0; m < M; ++m) {
    double q = 0.0;
    auto run = [&](auto sc) {
      constexpr int s = decltype(sc)::value;
      if (s < ST.n && ST.first[s < ST.n ? s : 0] < NT) {     // workgroup-uniform
        step(m, std::integral_constant<int, (s < ST.n ? s : 0)>{}, tsm + (pc & 1) * PIECE, tsm + ((pc & 1) ^ 1) * PIECE, q);
        ++pc;
      }
    };
    static_for<0, ST.n>(run);
    q += __shfl_xor(q, 16);
    q += __shfl_xor(q, 32);
    const double lc = lcv[m];
    if (lgrp == 0 && f < T) LP[f * ldy + m] = (lc == -INFINITY) ? -INFINITY : lc - 0.5 * q;
  }
}

// ------------------------------------------------------------------------------------------------
// (M,T) log-weighted densities -> posterior in place (MODE 0) or 1-based argmax (MODE 1).
// Lanes ACROSS the mixtures of a frame (8, 16, 32 or 64 of them: several frames per wave where M is small), so that a wave
// reads whole rows of the (T,M) matrix.  (Round 5: one lane per frame walked its row three times with a stride of M doubles
// between the lanes -- 1.47 ms for 5e5 x 64, fifteen times what the bytes take; tools/efficiency_sweep.py posterior.)
// Follows src/gmm.jl:28-29 (max-shifted log-sum-exp; exp(l - lse) evaluated as exp(l - max) / sum) and :46 (the FIRST maximum: ties go to the smaller index).
// ------------------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(256)
posterior_finish_kernel(double *__restrict__ LP, int M, int64_t T, int64_t *__restrict__ idx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lpf = M <= 8 ? 8 : (M <= 16 ? 16 : (M <= 32 ? 32 : 64)), fpw = 64 / lpf, sub = lane / lpf, sl = lane % lpf;
  for (int64_t f0 = ((int64_t)blockIdx.x * 4 + wave) * fpw; f0 < T; f0 += (int64_t)gridDim.x * 4 * fpw) {
    const int64_t fr = f0 + sub;
    const bool live = fr < T;
    double *l = LP + (live ? fr : T - 1) * M;
    // the lane's first maximum among m = sl, sl + lpf, ... (increasing m, strict >), then across the lanes
    double u = -INFINITY;
    int best = 0x7fffffff;
    if (sl < M) {
      u = l[sl];
      best = sl;
      for (int m = sl + lpf; m < M; m += lpf) {
        const double v = l[m];
        if (v > u) {
          u = v;
          best = m;
        }
      }
    }
    for (int o = lpf / 2; o >= 1; o >>= 1) {
      const double ou = __shfl_xor(u, o);
      const int ob = __shfl_xor(best, o);
      const bool take = ou > u || (ou == u && ob < best);
      u = take ? ou : u;
      best = take ? ob : best;
    }
    if (MODE == 1) {
      if (live && sl == 0) idx[fr] = best + 1;
      continue;
    }
    double s = 0.0;
    for (int m = sl; m < M; m += lpf) s += vc_exp(l[m] - u);
    for (int o = lpf / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    // exp(l - u) / s, not exp(l - (u + log s)): rounding lse = u + log s puts a common relative error of up to |lse| eps on every
    // posterior of the frame (rows of a 160-dimensional model summed to 1 within 58 eps only), the quotient one of 2 eps
    const double inv = 1.0 / s;
    if (live)
      for (int m = sl; m < M; m += lpf) l[m] = vc_exp(l[m] - u) * inv;
  }
}
static inline unsigned posterior_finish_grid(int M, int64_t T) {
  const int lpf = M <= 8 ? 8 : (M <= 16 ? 16 : (M <= 32 ? 32 : 64)), fpw = 64 / lpf;
  return (unsigned)std::min<int64_t>((T + 4 * fpw - 1) / (4 * fpw), 8192);
}

// ------------------------------------------------------------------------------------------------
// fvconvert for dimensions the MFMA tile kernel has no instantiation for (80 < padded D <= 160, e.g. the 82..96-dimensional
// static + delta vectors of 41..48 coefficients): log-weighted densities by logdens_tiled_kernel (MFMA), then this kernel --
// one wave per frame: softmax over the mixtures, and  y = sum_m p_m (A_m x + b_m)  over the mixtures whose posterior
// reaches e^-prune (the same rule as the tile kernel's pruning; prune = +inf: all of them), in mixture order.  A_m is read
// TRANSPOSED (At[m][k][d]: lanes along d are contiguous); x sits in LDS and is broadcast per k.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
convert_from_logdens_kernel(const double *__restrict__ LP, int M, int D, int DP, const double *__restrict__ At,
                            const double *__restrict__ b, const double *__restrict__ X, int64_t ldx, int64_t T,
                            double *__restrict__ Y, int64_t ldy, double prune) {
  __shared__ double xs_all[4][160];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double *xs = xs_all[wave];
  for (int64_t fr = (int64_t)blockIdx.x * 4 + wave; fr < T; fr += (int64_t)gridDim.x * 4) {
    const double *l = LP + fr * M;
    double u = -INFINITY;
    for (int m = lane; m < M; m += 64) u = fmax(u, l[m]);
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) u = fmax(u, __shfl_xor(u, sh));
    double sden = 0.0;
    for (int m0 = 0; m0 < M; m0 += 64) {        // fixed order: lanes' terms of a 64-mixture group summed by a butterfly
      double e = (m0 + lane < M) ? vc_exp(l[m0 + lane] - u) : 0.0;
#pragma unroll
      for (int sh = 1; sh < 64; sh <<= 1) e += __shfl_xor(e, sh);
      sden += e;
    }
    for (int k = lane; k < D; k += 64) xs[k] = X[fr * ldx + k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    for (int m = 0; m < M; ++m) {
      const double lm = l[m];                                   // wave-uniform (same address on every lane)
      if (!(lm > u - prune)) continue;
      const double p = vc_exp(lm - u) / sden;
      const double *am = At + (size_t)m * DP * DP + lane;
      double a0 = (lane < D) ? b[(size_t)m * DP + lane] : 0.0, a1 = (lane + 64 < D) ? b[(size_t)m * DP + lane + 64] : 0.0,
             a2 = (lane + 128 < D) ? b[(size_t)m * DP + lane + 128] : 0.0;
      for (int k = 0; k < D; ++k) {
        const double xk = xs[k];
        const double *row = am + (size_t)k * DP;
        if (lane < DP) a0 = fma(row[0], xk, a0);
        if (lane + 64 < DP) a1 = fma(row[64], xk, a1);
        if (lane + 128 < DP) a2 = fma(row[128], xk, a2);
      }
      y0 = fma(p, a0, y0);
      y1 = fma(p, a1, y1);
      y2 = fma(p, a2, y2);
    }
    if (lane < D) Y[fr * ldy + lane] = y0;
    if (lane + 64 < D) Y[fr * ldy + lane + 64] = y1;
    if (lane + 128 < D) Y[fr * ldy + lane + 128] = y2;
    __builtin_amdgcn_wave_barrier();                            // xs is rewritten for the wave's next frame
  }
}

template <int MODE>
static int launch_generic(const vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy,
                          hipStream_t st) {
  const size_t shmem = (size_t)g->D * 64 * sizeof(double) * (MODE == 0 ? 2 : 1);
  if (shmem > 160 * 1024) return fail(VCMI_ERR_ARG, "dimension %d too large for the generic kernel", g->D);
  auto kern = gmmmap_generic_kernel<MODE>;
  if (shmem > 64 * 1024)
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)shmem));
  const int64_t blocks = (T + 63) / 64;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64), shmem, st, g->U.p, g->A.p, g->cz.p, g->b.p, g->lc.p, g->M,
                     g->D, g->DP, dX, ldx, T, dY, ldy);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// ------------------------------------------------------------------------------------------------
// what gmmmap.hip launches (gmmmap_fallback.hpp)
// ------------------------------------------------------------------------------------------------
int gmmmap_generic_launch(const vcmi_gmmmap *g, int mode, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy,
                          hipStream_t st) {
  return mode == 0 ? launch_generic<0>(g, dX, ldx, T, dY, ldy, st) : launch_generic<1>(g, dX, ldx, T, dY, ldy, st);
}

int logdens_tiled_launch(const vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dLP, hipStream_t st) {
  constexpr int NTMAX = 10;
  constexpr TiledStages<NTMAX> ST{};
  const size_t shmem = 2 * (size_t)ST.max_piece() * sizeof(double);
  // (indexed by the handle's device, not the thread's current one: not the rule of set_max_dynamic_lds, vcmi_common.hpp)
  static std::atomic<bool> attr_done[64];
  if (!attr_done[g->device & 63].load(std::memory_order_acquire)) {
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(logdens_tiled_kernel<NTMAX>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    attr_done[g->device & 63].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL(logdens_tiled_kernel<NTMAX>, dim3((unsigned)((T + 127) / 128)), dim3(512), shmem, st, g->U.p, g->cz.p,
                     g->lc.p, g->M, g->D, g->DP, dX, ldx, T, dLP, (int64_t)g->M);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

int posterior_finish_launch(int mode, double *dLP, int M, int64_t T, int64_t *didx, hipStream_t st) {
  if (mode == 0) hipLaunchKernelGGL(posterior_finish_kernel<0>, dim3(posterior_finish_grid(M, T)), dim3(256), 0, st, dLP, M, T, didx);
  else hipLaunchKernelGGL(posterior_finish_kernel<1>, dim3(posterior_finish_grid(M, T)), dim3(256), 0, st, dLP, M, T, didx);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

int convert_from_logdens_launch(const vcmi_gmmmap *g, const double *dLP, const double *dX, int64_t ldx, int64_t T, double *dY,
                                int64_t ldy, hipStream_t st) {
  const unsigned blocks = (unsigned)std::min<int64_t>((T + 3) / 4, 16384);
  hipLaunchKernelGGL(convert_from_logdens_kernel, dim3(blocks), dim3(256), 0, st, dLP, g->M, g->D, g->DP, g->At.p, g->b.p, dX, ldx,
                     T, dY, ldy, g->prune);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

}  // namespace vcmi
