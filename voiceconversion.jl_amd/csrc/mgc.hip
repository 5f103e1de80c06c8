// mgc.hip -- the spectral-envelope transforms either side of a conversion (MelGeneralizedCepstrums, third party), MI355X
// (gfx950).
//
// Replaces   sp2mc(sp, order, alpha)    call sites test/vc.jl:16, bin/vc.jl:71, bin/mcep.jl:50
//            mc2sp(mc, alpha, fftlen)   call sites test/vc.jl:28, bin/vc.jl:87
//            mc2b(mc, alpha)            call sites test/diffvc.jl:33, bin/diffvc.jl:83
//
// sp2mc and mc2sp are each ONE fixed linear map between an elementwise log and an elementwise exp:
//   mc2sp:  log sp = G mc,        G = Cw F(-alpha)   ((fftlen/2+1) x D): freqt to fftlen/2, c[0] *= 2, the symmetric
//           vector's real FFT as a weighted cosine sum;
//   sp2mc:  mc = H log sp,        H = F(alpha) R     ((order+1) x K): R = the irfft of length N = 2(K-1) with row 0 halved,
//           then freqt over all N entries.
// Both matrices are built on the host in FP64 (cosine arguments reduced as integers k n mod N; freqt run over R as a block of
// columns), cached per thread keyed by (shape, alpha), and uploaded in v_mfma_f64_16x16x4_f64 fragment order, so each
// kernel is a GEMM over 16-frame tiles.  mc2b is a backward first-order recursion per frame (plain VALU).
#include "vcmi_common.hpp"
#include "fp64_exp.hpp"
#include "hostpipe.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace vcmi {

using d4 = __attribute__((__vector_size__(4 * sizeof(double)))) double;

static constexpr int kMgcMaxDim = 256;     // order + 1 and D
static constexpr int kMgcMaxBins = 4097;   // K = fftlen / 2 + 1 (fftlen <= 8192)
static constexpr int kMinChunkFrames = 4096;

// e^x over the whole double range: vc_exp's reduction and polynomial hold for |x| <= 1000 (n ln2_hi is exact for |n| < 2^21,
// ldexp overflows to +inf and underflows to 0 as Julia's exp does); NaN is passed through.
__device__ __forceinline__ double exp_full(double x) {
  const double y = vc_exp(fmin(x, 1000.0));
  return x != x ? x : y;
}

// ln x for positive finite x on the FP64 vector pipe: x = m 2^e with m in [sqrt(1/2), sqrt(2)), f = m - 1, s = f / (2 + f),
// ln(1 + f) = f - f^2/2 + s (f^2/2 + R(s^2)) with fdlibm's degree-7 polynomial R (|s| <= 0.1716, error below 2^-58), the
// quotient from v_rcp_f64 and two Newton steps.  About 30 instructions, a third of the library log's extra-precise
// evaluation -- the log is the larger half of sp2mc's FP64 pipe work.  0 gives -inf, +inf gives +inf, anything else that
// is not positive (or NaN) gives NaN, as the library log does.
__device__ __forceinline__ double log_pos(double x) {
  double m = __builtin_amdgcn_frexp_mant(x);              // [0.5, 1)
  int e = __builtin_amdgcn_frexp_exp(x);
  if (m < 0.70710678118654752440) {
    m += m;
    --e;
  }
  const double f = m - 1.0;                               // exact
  const double d = 2.0 + f;
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.0), r, r);
  r = fma(fma(-d, r, 1.0), r, r);
  double sq = f * r;
  sq = fma(fma(-d, sq, f), r, sq);                        // s = f / (2 + f)
  const double z = sq * sq;
  double R = vc_fma_sconst(1.479819860511658591e-01, z, 1.531383769920937332e-01);
  R = vc_fma_sconst(R, z, 1.818357216161805012e-01);
  R = vc_fma_sconst(R, z, 2.222219843214978396e-01);
  R = vc_fma_sconst(R, z, 2.857142874366239149e-01);
  R = vc_fma_sconst(R, z, 3.999999999940941908e-01);
  R = vc_fma_sconst(R, z, 6.666666666666735130e-01);
  R *= z;
  const double hfsq = 0.5 * f * f;
  const double k = (double)e;
  const double lo = fma(sq, hfsq + R, k * 1.90821492927058770002e-10);
  const double y = fma(k, 6.93147180369123816490e-01, f - (hfsq - lo));
  if (x > 0.0 && x <= 1.79769313486231570815e+308) return y;
  return x == 0.0 ? -__builtin_inf() : x > 0.0 ? x : __builtin_nan("");   // log 0 = -inf, log inf = inf, else NaN
}

// ------------------------------------------------------------------------------------------------------------------------
// mc2sp: sp[k, t] = exp(sum_d G[k, d] mc[d, t]).  One wave = RBW consecutive 16-row blocks of G, resident in registers
// (KS = ceil(D/4) fragments each), walking the 16-frame tiles of its frame group: one load of a tile's mel-cepstra feeds the
// RBW MFMA chains, and the next tile's load is in flight while the current one is computed.  Gf[rb][ks][lane] =
// G[16 rb + (lane & 15)][4 ks + (lane >> 4)] (zero outside).  The exps go through a per-wave LDS tile ([frame][row],
// 16 RBW rows per frame, padded) so that each store instruction writes 16 RBW contiguous rows of ONE frame (512 bytes at
// RBW = 4, 384 at 3) instead of 32-byte pieces of 16 frames.
// Work items (row group, frame group) are numbered so that the row groups of one frame group run on one XCD (dispatch is
// round robin over the 8 XCDs): the tile a wave reads is then in the L2 its neighbours just filled.
template <int KSMAX, int RBW>
__global__ void __launch_bounds__(256)
mc2sp_kernel(const double *__restrict__ Gf, int K, int KS, int RGW, int FG, const double *__restrict__ mc, int64_t ldm, int D,
             int64_t T, double *__restrict__ sp, int64_t lds) {
  constexpr int ROWS = 16 * RBW, S = ROWS + 4;             // LDS row stride: 2-way bank sharing on the transposed writes
  __shared__ double tr[4][16 * S];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lcol = lane & 15, lgrp = lane >> 4;
  const int nb = gridDim.x;                                // a multiple of 8
  const int b = blockIdx.x;
  const int task = ((b & 7) * (nb >> 3) + (b >> 3)) * 4 + wave;
  if (task >= RGW * FG) return;
  const int rg = task % RGW, fg = task / RGW;
  const int k0 = rg * ROWS;
  const int nrow = min(ROWS, K - k0);
  double *w = tr[wave];
  double a[RBW][KSMAX];
#pragma unroll
  for (int q = 0; q < RBW; ++q)
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks)
      if (ks < KS) a[q][ks] = (16 * q < nrow) ? Gf[((size_t)(rg * RBW + q) * KS + ks) * 64 + lane] : 0.0;
  const int64_t ntiles = (T + 15) / 16;
  double xn[KSMAX];
  auto load = [&](int64_t tile) {
    const int64_t t = tile * 16 + lcol;
    const bool tv = tile < ntiles && t < T;
    const double *col = mc + (tv ? t : 0) * ldm;
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks)
      if (ks < KS) {
        const int d = 4 * ks + lgrp;
        xn[ks] = (tv && d < D) ? col[d] : 0.0;
      }
  };
  load(fg);
  for (int64_t tile = fg; tile < ntiles; tile += FG) {
    double x[KSMAX];
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks) x[ks] = xn[ks];
    load(tile + FG);
    d4 acc[RBW];
#pragma unroll
    for (int q = 0; q < RBW; ++q) {
      acc[q] = d4{0.0, 0.0, 0.0, 0.0};
      if (16 * q < nrow) {
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks)
          if (ks < KS) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q][ks], x[ks], acc[q], 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < RBW; ++q)
      if (16 * q < nrow)
#pragma unroll
        for (int r = 0; r < 4; ++r) w[lcol * S + 16 * q + lgrp + 4 * r] = exp_full(acc[q][r]);
    __builtin_amdgcn_wave_barrier();
    const int nf = (int)min<int64_t>(16, T - tile * 16);
    double *out = sp + tile * 16 * lds + k0;
    for (int f = 0; f < nf; ++f)
      for (int rr = lane; rr < nrow; rr += 64) out[f * lds + rr] = w[f * S + rr];
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// sp2mc: mc[d, t] = sum_k H[d, k] log sp[k, t].  One wave = FT 16-frame tiles, every output row (MB = ceil((order+1)/16)
// accumulators per tile); the workgroup's four waves stream H through LDS in chunks of KC k-steps.  Each lane computes the
// log of one input element per k-step and tile, which feeds all MB MFMA chains of that tile.
// The input is read in 32-byte pieces: in a group of four k-steps (16 bins) lane (lgrp, lcol) holds bins
// 16 b + 4 lgrp + s, s = 0..3, of frame lcol, and k-step 4 b + s uses piece element s -- the k order of the MFMA is free, so
// H is laid out to match: Hf[ks][mb][lane] = H[16 mb + (lane & 15)][16 (ks / 4) + 4 (lane >> 4) + ks % 4] (zero outside;
// KS and KC multiples of 4, so a chunk is one contiguous range).  Each group of four load instructions reads 128
// contiguous bytes of each of the wave's frames.
// bad (optional): set to 1 when an input entry of a real frame is not positive and finite (host entry's argument check).
template <int MBMAX, int FT>
__global__ void __launch_bounds__(256)
sp2mc_kernel(const double *__restrict__ Hf, int M1, int MB, int KS, int KC, const double *__restrict__ sp, int64_t lds, int K,
             int64_t T, double *__restrict__ mc, int64_t ldm, int *__restrict__ bad) {
  typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));
  extern __shared__ double hs[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lcol = lane & 15, lgrp = lane >> 4;
  const int64_t t0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * FT);
  const double *col[FT];
  bool tv[FT];
#pragma unroll
  for (int f = 0; f < FT; ++f) {
    const int64_t t = t0 + 16 * f + lcol;
    tv[f] = t < T;
    col[f] = sp + (tv[f] ? t : 0) * lds;
  }
  d4 acc[FT][MBMAX];
#pragma unroll
  for (int f = 0; f < FT; ++f)
#pragma unroll
    for (int mb = 0; mb < MBMAX; ++mb) acc[f][mb] = d4{0.0, 0.0, 0.0, 0.0};
  bool wrong = false;
  for (int c0 = 0; c0 < KS; c0 += KC) {
    const int nks = min(KC, KS - c0);
    __syncthreads();
    {
      const double *src = Hf + (size_t)c0 * MB * 64;
      const int n = nks * MB * 64;
      for (int i = threadIdx.x; i < n; i += 256) hs[i] = src[i];
    }
    __syncthreads();
    for (int j = 0; j < nks; j += 4) {
      const int k = 4 * (c0 + j) + 4 * lgrp;              // first bin of this lane's piece
      double v[FT][4];
#pragma unroll
      for (int f = 0; f < FT; ++f) {
        if (tv[f] && k + 3 < K) {
          const d2u p = *reinterpret_cast<const d2u *>(col[f] + k), q = *reinterpret_cast<const d2u *>(col[f] + k + 2);
          v[f][0] = p.x;
          v[f][1] = p.y;
          v[f][2] = q.x;
          v[f][3] = q.y;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[f][e] = (tv[f] && k + e < K) ? col[f][k + e] : 1.0;   // log 1 = 0: padding
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          wrong |= !(v[f][e] > 0.0 && v[f][e] <= 1.79769313486231570815e+308);
          v[f][e] = log_pos(v[f][e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double *hj = hs + (size_t)(j + e) * MB * 64 + lane;
#pragma unroll
        for (int mb = 0; mb < MBMAX; ++mb)
          if (mb < MB) {
            const double a = hj[mb * 64];
#pragma unroll
            for (int f = 0; f < FT; ++f) acc[f][mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, v[f][e], acc[f][mb], 0, 0, 0);
          }
      }
    }
  }
  if (bad && wrong) *bad = 1;
#pragma unroll
  for (int f = 0; f < FT; ++f) {
    if (!tv[f]) continue;
    double *out = mc + (t0 + 16 * f + lcol) * ldm;
#pragma unroll
    for (int mb = 0; mb < MBMAX; ++mb)
      if (mb < MB)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int d = 16 * mb + lgrp + 4 * r;
          if (d < M1) out[d] = acc[f][mb][r];
        }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// mc2b: b[D-1] = mc[D-1], b[i] = mc[i] - alpha b[i+1]; one thread per frame.  (b may be mc: each entry is read before it is
// written, by the same thread.)
__global__ void __launch_bounds__(256)
mc2b_kernel(const double *mc, int64_t ldm, int D, int64_t T, double alpha, double *b, int64_t ldb) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (int64_t)gridDim.x * 256) {
    const double *x = mc + t * ldm;
    double *y = b + t * ldb;
    double v = x[D - 1];
    y[D - 1] = v;
    for (int i = D - 2; i >= 0; --i) {
      v = x[i] - alpha * v;
      y[i] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// Host: the folded matrices.

// freqt (SPTK recursion) of the columns of `in` (m1+1 rows of ncol columns, row-major: in[i * ncol + c]) to m2+1 rows with
// warping parameter a: out[j * ncol + c].  The recursion runs over a block of columns at once.
static void freqt_block(const double *in, int m1, int ncol, int m2, double a, double *out) {
  const double b = 1.0 - a * a;
  std::vector<double> g((size_t)(m2 + 1) * ncol, 0.0), d((size_t)(m2 + 1) * ncol);
  for (int i = m1; i >= 0; --i) {
    d.swap(g);
    const double *ci = in + (size_t)i * ncol;
    for (int c = 0; c < ncol; ++c) g[c] = ci[c] + a * d[c];
    if (m2 >= 1)
      for (int c = 0; c < ncol; ++c) g[ncol + c] = b * d[c] + a * d[ncol + c];
    for (int j = 2; j <= m2; ++j) {
      double *gj = &g[(size_t)j * ncol];
      const double *gm = &g[(size_t)(j - 1) * ncol], *dj = &d[(size_t)j * ncol], *dm = &d[(size_t)(j - 1) * ncol];
      for (int c = 0; c < ncol; ++c) gj[c] = dm[c] + a * (dj[c] - gm[c]);
    }
  }
  std::copy(g.begin(), g.end(), out);
}

// cos(2 pi j / N) for j = 0 .. N-1, from the integer residue (callers reduce k n mod N first)
static std::vector<double> cos_table(int N) {
  std::vector<double> c((size_t)N);
  const long double w = 2.0L * 3.141592653589793238462643383279502884L / (long double)N;
  for (int j = 0; j < N; ++j) c[j] = (double)cosl(w * (long double)j);
  return c;
}

// G = Cw F(-alpha), (K x D) with K = fftlen/2 + 1, in fragment order Gf[rb][ks][64]
static void build_mc2sp_matrix(int D, double alpha, int fftlen, std::vector<double> &Gf) {
  const int L = fftlen / 2, K = L + 1, KS = (D + 3) / 4, RB = (K + 15) / 16;
  std::vector<double> eye((size_t)D * D, 0.0), F((size_t)(L + 1) * D);   // F[n][d]
  for (int d = 0; d < D; ++d) eye[(size_t)d * D + d] = 1.0;
  freqt_block(eye.data(), D - 1, D, L, -alpha, F.data());
  const std::vector<double> cs = cos_table(fftlen);
  std::vector<double> w((size_t)L + 1, 2.0);
  if (fftlen % 2 == 0) w[L] = 1.0;                          // s[L] is one entry of the symmetric vector when fftlen is even
  Gf.assign((size_t)RB * KS * 64, 0.0);
  host_parallel_for(K, 16, [&](int64_t lo, int64_t hi) {
    std::vector<double> row((size_t)D);
    for (int64_t k = lo; k < hi; ++k) {
      std::fill(row.begin(), row.end(), 0.0);
      for (int n = 0; n <= L; ++n) {
        const double c = w[n] * cs[(size_t)((int64_t)k * n % fftlen)];
        const double *fn = &F[(size_t)n * D];
        for (int d = 0; d < D; ++d) row[d] += c * fn[d];
      }
      const int rb = (int)(k / 16), i = (int)(k % 16);
      for (int d = 0; d < D; ++d) Gf[((size_t)rb * KS + d / 4) * 64 + (d % 4) * 16 + i] = row[d];
    }
  });
}

static int sp2mc_ksteps(int K) { return (K + 15) / 16 * 4; }   // k-steps of sp2mc_kernel: whole groups of four

// H = F(alpha) R, ((order+1) x K), R[n][k] = w_k cos(2 pi k n / N) / N (row 0 halved), N = 2(K-1); fragment order
// Hf[ks][mb][64]
static void build_sp2mc_matrix(int K, int order, double alpha, std::vector<double> &Hf) {
  const int N = 2 * (K - 1), M1 = order + 1, KS = sp2mc_ksteps(K), MB = (M1 + 15) / 16;
  const std::vector<double> cs = cos_table(N);
  Hf.assign((size_t)KS * MB * 64, 0.0);
  const int64_t kblk = 32;                                  // columns of R per freqt block
  host_parallel_for((K + kblk - 1) / kblk, 1, [&](int64_t lo, int64_t hi) {
    for (int64_t blk = lo; blk < hi; ++blk) {
      const int c0 = (int)(blk * kblk), nc = std::min<int>((int)kblk, K - c0);
      std::vector<double> R((size_t)N * nc), H((size_t)M1 * nc);
      for (int n = 0; n < N; ++n)
        for (int c = 0; c < nc; ++c) {
          const int k = c0 + c;
          const double wk = (k == 0 || k == K - 1) ? 1.0 : 2.0;
          R[(size_t)n * nc + c] = wk * cs[(size_t)((int64_t)k * n % N)] / (double)N * (n == 0 ? 0.5 : 1.0);
        }
      freqt_block(R.data(), N - 1, nc, order, alpha, H.data());
      for (int m = 0; m < M1; ++m)
        for (int c = 0; c < nc; ++c) {
          const int k = c0 + c;
          const int ks = 4 * (k / 16) + k % 4, kg = (k % 16) / 4;   // bin k = 16 (ks / 4) + 4 kg + ks % 4
          Hf[((size_t)ks * MB + m / 16) * 64 + kg * 16 + m % 16] = H[(size_t)m * nc + c];
        }
    }
  });
}

struct MgcScratch {
  DevBuf<double> G, H;
  DevBuf<int> flag;
  int g_D = 0, g_fftlen = 0, h_K = 0, h_order = 0;
  double g_alpha = 0.0, h_alpha = 0.0;
  StreamOrder order;
};
static MgcScratch &mscratch() {
  static thread_local MgcScratch s;
  return s;
}

static int ensure_mc2sp(MgcScratch &sc, int D, double alpha, int fftlen) {
  if (sc.G.p && sc.g_D == D && sc.g_fftlen == fftlen && sc.g_alpha == alpha) return VCMI_OK;
  std::vector<double> Gf;
  build_mc2sp_matrix(D, alpha, fftlen, Gf);
  VCMI_HIP(hipDeviceSynchronize());                         // an earlier call's kernel may still read the old matrix
  VCMI_TRY(sc.G.reserve(Gf.size()));
  VCMI_TRY(upload_now(sc.G.p, Gf.data(), Gf.size() * 8));
  sc.g_D = D;
  sc.g_fftlen = fftlen;
  sc.g_alpha = alpha;
  return VCMI_OK;
}

static int ensure_sp2mc(MgcScratch &sc, int K, int order, double alpha) {
  if (sc.H.p && sc.h_K == K && sc.h_order == order && sc.h_alpha == alpha) return VCMI_OK;
  std::vector<double> Hf;
  build_sp2mc_matrix(K, order, alpha, Hf);
  VCMI_HIP(hipDeviceSynchronize());
  VCMI_TRY(sc.H.reserve(Hf.size()));
  VCMI_TRY(upload_now(sc.H.p, Hf.data(), Hf.size() * 8));
  sc.h_K = K;
  sc.h_order = order;
  sc.h_alpha = alpha;
  return VCMI_OK;
}

static int mc2sp_launch(const MgcScratch &sc, const double *dmc, int64_t ldm, int D, int64_t T, int fftlen, double *dsp,
                        int64_t lds, hipStream_t st) {
  if (T == 0) return VCMI_OK;
  const int K = fftlen / 2 + 1, KS = (D + 3) / 4, RB = (K + 15) / 16;
  const int RBW = KS <= 12 ? 3 : KS <= 24 ? 2 : 1;          // row blocks per wave (3 at D <= 48: 2.44 ms against 2.52 with 4)
  const int RGW = (RB + RBW - 1) / RBW;
  const int64_t ntiles = (T + 15) / 16;
  // about 6000 waves in all, whole frame groups (measured at D = 41, K = 513: 2048 / 3072 / 6144 waves 3.6 / 2.7 / 2.4 ms)
  const int FG = (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, (6144 + RGW - 1) / RGW));
  const int64_t tasks = (int64_t)RGW * FG;
  const dim3 grid((unsigned)((tasks + 31) / 32 * 8)), block(256);   // 4 waves per workgroup, workgroups a multiple of 8
#define VCMI_MC2SP(KSM, R)                                                                                             \
  hipLaunchKernelGGL((mc2sp_kernel<KSM, R>), grid, block, 0, st, sc.G.p, K, KS, RGW, FG, dmc, ldm, D, T, dsp, lds)
  if (KS <= 4) VCMI_MC2SP(4, 3);
  else if (KS <= 8) VCMI_MC2SP(8, 3);
  else if (KS <= 12) VCMI_MC2SP(12, 3);
  else if (KS <= 16) VCMI_MC2SP(16, 2);
  else if (KS <= 24) VCMI_MC2SP(24, 2);
  else if (KS <= 32) VCMI_MC2SP(32, 1);
  else if (KS <= 48) VCMI_MC2SP(48, 1);
  else VCMI_MC2SP(64, 1);
#undef VCMI_MC2SP
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

static int sp2mc_launch(const MgcScratch &sc, const double *dsp, int64_t lds, int K, int64_t T, int order, double *dmc,
                        int64_t ldm, int *bad, hipStream_t st) {
  if (T == 0) return VCMI_OK;
  const int M1 = order + 1, MB = (M1 + 15) / 16, KS = sp2mc_ksteps(K);
  const int KC = std::max(4, 64 / MB / 4 * 4);              // k-steps per LDS chunk (whole groups): at most 32 KB of H
  const size_t shm = (size_t)std::min(KC, KS) * MB * 64 * sizeof(double);
  const int FT = MB <= 4 ? 2 : 1;
  const int64_t blocks = (T + 64 * FT - 1) / (64 * FT);
  const dim3 grid((unsigned)blocks), block(256);
#define VCMI_SP2MC(MBM, F)                                                                                             \
  hipLaunchKernelGGL((sp2mc_kernel<MBM, F>), grid, block, shm, st, sc.H.p, M1, MB, KS, KC, dsp, lds, K, T, dmc, ldm, bad)
  if (MB == 1) VCMI_SP2MC(1, 2);
  else if (MB == 2) VCMI_SP2MC(2, 2);
  else if (MB == 3) VCMI_SP2MC(3, 2);
  else if (MB == 4) VCMI_SP2MC(4, 2);
  else if (MB <= 6) VCMI_SP2MC(6, 1);
  else if (MB <= 8) VCMI_SP2MC(8, 1);
  else if (MB <= 12) VCMI_SP2MC(12, 1);
  else VCMI_SP2MC(16, 1);
#undef VCMI_SP2MC
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

static int mc2b_launch(const double *dmc, int64_t ldm, int D, int64_t T, double alpha, double *db, int64_t ldb, hipStream_t st) {
  if (T == 0) return VCMI_OK;
  const int64_t blocks = std::min<int64_t>((T + 255) / 256, 8192);
  hipLaunchKernelGGL(mc2b_kernel, dim3((unsigned)blocks), dim3(256), 0, st, dmc, ldm, D, T, alpha, db, ldb);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

static int check_alpha(double alpha, const char *who) {
  if (!(std::fabs(alpha) < 1.0)) return fail(VCMI_ERR_ARG, "%s: |alpha| = %g must be below 1", who, std::fabs(alpha));
  return VCMI_OK;
}

static int check_sp2mc(int K, int64_t T, int order, double alpha, const char *who) {
  if (K < 2 || K > kMgcMaxBins || T < 0 || order < 0 || order + 1 > kMgcMaxDim)
    return fail(VCMI_ERR_DIM, "%s: K=%d T=%lld order=%d unsupported (needs 2 <= K <= %d, 0 <= order < %d, T >= 0)", who, K,
                (long long)T, order, kMgcMaxBins, kMgcMaxDim);
  return check_alpha(alpha, who);
}

static int check_mc2sp(int D, int64_t T, double alpha, int fftlen, const char *who) {
  if (D < 1 || D > kMgcMaxDim || T < 0)
    return fail(VCMI_ERR_DIM, "%s: D=%d T=%lld unsupported (needs 1 <= D <= %d, T >= 0)", who, D, (long long)T, kMgcMaxDim);
  if (fftlen < 2 || fftlen / 2 + 1 > kMgcMaxBins)
    return fail(VCMI_ERR_ARG, "%s: fftlen=%d unsupported (needs 2 <= fftlen <= %d)", who, fftlen, 2 * (kMgcMaxBins - 1) + 1);
  return check_alpha(alpha, who);
}

}  // namespace vcmi

using namespace vcmi;

// sp2mc(sp, order, alpha) for every column of sp (K,T) -> mc (order+1,T); call sites test/vc.jl:16, bin/vc.jl:71, bin/mcep.jl:50
extern "C" int vcmi_sp2mc(const double *sp, int K, int64_t T, int order, double alpha, double *mc) {
  if (!sp || !mc) return fail(VCMI_ERR_ARG, "vcmi_sp2mc: NULL argument");
  VCMI_TRY(check_sp2mc(K, T, order, alpha, "vcmi_sp2mc"));
  if (T == 0) return VCMI_OK;
  VCMI_TRY(check_device());
  MgcScratch &sc = mscratch();
  VCMI_TRY(ensure_sp2mc(sc, K, order, alpha));
  VCMI_TRY(sc.flag.reserve(1));
  VCMI_HIP(hipMemset(sc.flag.p, 0, sizeof(int)));
  const int M1 = order + 1;
  // the argument check rides on the kernel's log prologue: every entry is tested where it is read, no extra pass
  VCMI_TRY(staged_pipeline(sp, (size_t)K * 8, (size_t)K * 8, mc, (size_t)M1 * 8, (size_t)M1 * 8, T, kMinChunkFrames,
                           [&](const void *dIn, void *dOut, int64_t, int64_t n, hipStream_t st) -> int {
                             return sp2mc_launch(sc, (const double *)dIn, K, K, n, order, (double *)dOut, M1, sc.flag.p, st);
                           }));
  int bad = 0;
  VCMI_HIP(hipMemcpy(&bad, sc.flag.p, sizeof(int), hipMemcpyDeviceToHost));
  if (bad) return fail(VCMI_ERR_ARG, "vcmi_sp2mc: the spectrum has entries that are not positive and finite");
  return VCMI_OK;
}

extern "C" int vcmi_sp2mc_dev(const double *dsp, int64_t lds, int K, int64_t T, int order, double alpha, double *dmc,
                              int64_t ldm, void *stream) {
  if (!dsp || !dmc) return fail(VCMI_ERR_ARG, "vcmi_sp2mc_dev: NULL argument");
  VCMI_TRY(check_sp2mc(K, T, order, alpha, "vcmi_sp2mc_dev"));
  if (lds < K || ldm < order + 1) return fail(VCMI_ERR_ARG, "vcmi_sp2mc_dev: leading dimension below the column length");
  if (T == 0) return VCMI_OK;
  VCMI_TRY(check_device());
  MgcScratch &sc = mscratch();
  const hipStream_t st = as_stream(stream);
  VCMI_TRY(ensure_sp2mc(sc, K, order, alpha));
  VCMI_TRY(sc.order.enter(st));
  VCMI_TRY(sp2mc_launch(sc, dsp, lds, K, T, order, dmc, ldm, nullptr, st));
  return sc.order.leave(st);
}

// mc2sp(mc, alpha, fftlen) for every column of mc (D,T) -> sp (fftlen/2+1,T); call sites test/vc.jl:28, bin/vc.jl:87
extern "C" int vcmi_mc2sp(const double *mc, int D, int64_t T, double alpha, int fftlen, double *sp) {
  if (!mc || !sp) return fail(VCMI_ERR_ARG, "vcmi_mc2sp: NULL argument");
  VCMI_TRY(check_mc2sp(D, T, alpha, fftlen, "vcmi_mc2sp"));
  if (T == 0) return VCMI_OK;
  VCMI_TRY(check_device());
  MgcScratch &sc = mscratch();
  VCMI_TRY(ensure_mc2sp(sc, D, alpha, fftlen));
  const int K = fftlen / 2 + 1;
  return staged_pipeline(mc, (size_t)D * 8, (size_t)D * 8, sp, (size_t)K * 8, (size_t)K * 8, T, kMinChunkFrames,
                         [&](const void *dIn, void *dOut, int64_t, int64_t n, hipStream_t st) -> int {
                           return mc2sp_launch(sc, (const double *)dIn, D, D, n, fftlen, (double *)dOut, K, st);
                         });
}

extern "C" int vcmi_mc2sp_dev(const double *dmc, int64_t ldm, int D, int64_t T, double alpha, int fftlen, double *dsp,
                              int64_t lds, void *stream) {
  if (!dmc || !dsp) return fail(VCMI_ERR_ARG, "vcmi_mc2sp_dev: NULL argument");
  VCMI_TRY(check_mc2sp(D, T, alpha, fftlen, "vcmi_mc2sp_dev"));
  if (ldm < D || lds < fftlen / 2 + 1) return fail(VCMI_ERR_ARG, "vcmi_mc2sp_dev: leading dimension below the column length");
  if (T == 0) return VCMI_OK;
  VCMI_TRY(check_device());
  MgcScratch &sc = mscratch();
  const hipStream_t st = as_stream(stream);
  VCMI_TRY(ensure_mc2sp(sc, D, alpha, fftlen));
  VCMI_TRY(sc.order.enter(st));
  VCMI_TRY(mc2sp_launch(sc, dmc, ldm, D, T, fftlen, dsp, lds, st));
  return sc.order.leave(st);
}

// mc2b(mc, alpha) for every column of mc (D,T) -> b (D,T); call sites test/diffvc.jl:33, bin/diffvc.jl:83
extern "C" int vcmi_mc2b(const double *mc, int D, int64_t T, double alpha, double *b) {
  if (!mc || !b) return fail(VCMI_ERR_ARG, "vcmi_mc2b: NULL argument");
  if (D < 1 || T < 0) return fail(VCMI_ERR_DIM, "vcmi_mc2b: D=%d T=%lld invalid", D, (long long)T);
  VCMI_TRY(check_alpha(alpha, "vcmi_mc2b"));
  if (T == 0) return VCMI_OK;
  VCMI_TRY(check_device());
  return staged_pipeline(mc, (size_t)D * 8, (size_t)D * 8, b, (size_t)D * 8, (size_t)D * 8, T, kMinChunkFrames,
                         [&](const void *dIn, void *dOut, int64_t, int64_t n, hipStream_t st) -> int {
                           return mc2b_launch((const double *)dIn, D, D, n, alpha, (double *)dOut, D, st);
                         });
}

extern "C" int vcmi_mc2b_dev(const double *dmc, int64_t ldm, int D, int64_t T, double alpha, double *db, int64_t ldb,
                             void *stream) {
  if (!dmc || !db) return fail(VCMI_ERR_ARG, "vcmi_mc2b_dev: NULL argument");
  if (D < 1 || T < 0) return fail(VCMI_ERR_DIM, "vcmi_mc2b_dev: D=%d T=%lld invalid", D, (long long)T);
  VCMI_TRY(check_alpha(alpha, "vcmi_mc2b_dev"));
  if (ldm < D || ldb < D) return fail(VCMI_ERR_ARG, "vcmi_mc2b_dev: leading dimension below D");
  if (T == 0) return VCMI_OK;
  VCMI_TRY(check_device());
  return mc2b_launch(dmc, ldm, D, T, alpha, db, ldb, as_stream(stream));
}
