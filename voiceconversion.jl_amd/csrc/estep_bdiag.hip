// estep_bdiag.hip -- E-step of a CROSS-DIAGONAL ("block_diag") joint GMM, MI355X (gfx950): vcmi_estep_bdiag_dev and the
// E-step of vcmi_gmm_em_bdiag_* (gmm_em.hip).
//
// The model (Toda, Black, Tokuda 2007): each of the four blocks of the joint covariance is diagonal, so joint row d couples
// with row d + D only (D = Dj / 2) -- a 2 x 2 block [vx c; c vy] per pair.  Parameter block, on the device:
//   raw = [w (M) | mu (Dj,M) | covars (Dj + D, M)],  covars[:, m] = [var (Dj) | c (D)].
// Three kernels per chunk of frames, one code path for every even Dj <= 256 and M <= 256 (run-time loops):
//   * estep_bdiag_prep_kernel: per pair the conditional factorisation of its 2 x 2 block and the validity check, per mixture
//     the constant log w - (Dj log 2 pi + sum log det) / 2 (a fixed-order tree);
//   * estep_bdiag_gamma_kernel (phase 1): log-densities in the CENTRED form on the vector pipe, the softmax, gamma
//     (frames x M) and per-workgroup log-likelihood partials to HBM;
//   * estep_bdiag_stats_kernel (phase 2): gamma' [z, z^2, x.y] on v_mfma_f64_16x16x4_f64, per (16 mixtures, 16 pairs, segment
//     of frames); per-segment partial rows, summed in a fixed order by estep_reduce_kernel.
// No floating-point atomics anywhere: identical inputs give identical bits whatever ran before.
#include "estep_internal.hpp"
#include "hostpipe.hpp"

#include <climits>
#include <cmath>

namespace vcmi {

static constexpr double kBdLog2Pi = 1.8378770664093454835606594728112;
typedef double d4 __attribute__((ext_vector_type(4)));

static constexpr int kBdFB = 64;            // frames per phase-1 workgroup (lane = frame)
static constexpr int kBdRS = kBdFB + 1;     // row stride of the transposed frame tile in LDS (odd: the staging writes spread over the banks)
static constexpr int kBdSeg = 1024;         // frames per phase-2 segment = per partial row
static constexpr int kBdChunk = 1 << 17;    // frames per pass of the two phases (bounds gamma: 2^17 M doubles)
static constexpr int kBdPrm = 5;            // doubles per (mixture, pair) of the prepared model
static constexpr int kBdGammaThreads = 512; // phase 1: eight waves share one frame tile

// per pair (d, m): [mu_x, mu_y, b = c / vx, 1 / vx, vx / det]: the quadratic form of the pair is
//   dx^2 / vx + (dy - b dx)^2 vx / det      (= (vy dx^2 - 2 c dx dy + vx dy^2) / det, without its cancellation at |rho| -> 1)
__global__ void __launch_bounds__(128)
estep_bdiag_prep_kernel(const double *__restrict__ raw, int Dj, int M, double *__restrict__ prm, double *__restrict__ cst,
                        int *__restrict__ flag) {
  __shared__ double red[128];
  const int D = Dj / 2, m = blockIdx.x, d = threadIdx.x;
  const double *mu = raw + M + (size_t)m * Dj, *cv = raw + M + (size_t)M * Dj + (size_t)m * (Dj + D);
  double ld = 0.0;
  if (d < D) {
    const double vx = cv[d], vy = cv[D + d], c = cv[Dj + d];
    const double det = bdiag_det(vx, vy, c);
    if (!bdiag_pair_valid(vx, vy, c)) atomicMin(flag, 1 + d + D * m);     // (an integer minimum: the first in memory order)
    double *p = prm + ((size_t)m * D + d) * kBdPrm;
    p[0] = mu[d];
    p[1] = mu[D + d];
    p[2] = c / vx;
    p[3] = 1.0 / vx;
    p[4] = vx / det;
    ld = log(det);
  }
  red[d] = ld;
  __syncthreads();
  for (int o = 64; o >= 1; o >>= 1) {
    if (d < o) red[d] += red[d + o];
    __syncthreads();
  }
  if (d == 0) cst[m] = log(raw[m]) - 0.5 * (Dj * kBdLog2Pi + red[0]);
}

// PHASE 1.  64 frames per workgroup, transposed into LDS (xs[row][frame]); lane = frame, wave w of the eight takes the mixtures
// 4 w .. 4 w + 3, then + 32, ...: one pair of LDS reads serves four mixtures, whose parameters are wave-uniform (scalar loads).
// (Eight waves on one tile: the tile is what limits the workgroups of a CU -- 83 KB at Dj = 160 -- so the waves that hide the
// scalar-load latency have to come from the workgroup.)  The log-densities go to G, then four threads per frame (the first
// four waves) turn them into responsibilities in place (maximum, sum and log-sum-exp by butterflies inside the quad: the same
// bits in its four lanes).  llpart[workgroup] = sum of its frames' log-sum-exps, in a fixed order.  G is chunk-local: row f
// of G is frame n0 + f of X.
__global__ void __launch_bounds__(kBdGammaThreads)
estep_bdiag_gamma_kernel(const double *__restrict__ X, int64_t n0, int64_t nfr, int Dj, int M, const double *__restrict__ prm,
                         const double *__restrict__ cst, double *__restrict__ G, double *__restrict__ llpart) {
  extern __shared__ double xs[];   // [Dj][kBdRS]
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = Dj / 2;
  const int64_t f0 = (int64_t)blockIdx.x * kBdFB;
  const int nf = (int)((nfr - f0 < kBdFB) ? nfr - f0 : kBdFB);
  const double *src = X + (size_t)(n0 + f0) * Dj;      // the workgroup's frames are contiguous
  for (int i = tid; i < kBdFB * Dj; i += kBdGammaThreads) {
    const int f = i / Dj, d = i - f * Dj;
    xs[d * kBdRS + f] = (f < nf) ? src[i] : 0.0;
  }
  __syncthreads();
  {
    double *g = G + (size_t)(f0 + lane) * M;
    for (int mw = 4 * wave; mw < M; mw += kBdGammaThreads / 16) {
      const int m0 = __builtin_amdgcn_readfirstlane(mw);
      const double *p[4];
      double q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int j = 0; j < 4; ++j) p[j] = prm + (size_t)((m0 + j < M) ? m0 + j : M - 1) * D * kBdPrm;
      for (int d = 0; d < D; ++d) {
        const double x = xs[d * kBdRS + lane], y = xs[(D + d) * kBdRS + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double *pp = p[j] + d * kBdPrm;
          const double dx = x - pp[0], dy = y - pp[1];
          const double e = fma(-pp[2], dx, dy);
          q[j] = fma(dx * dx, pp[3], q[j]);
          q[j] = fma(e * e, pp[4], q[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (lane < nf && m0 + j < M) g[m0 + j] = cst[m0 + j] - 0.5 * q[j];
    }
  }
  __syncthreads();      // (orders the workgroup's global writes of G before the reads below)
  const int f = tid >> 2, qd = tid & 3;
  const bool live = f < nf;             // (f >= 64 in the waves 4 .. 7: they only wait at the last barrier)
  double *gf = G + (size_t)(f0 + f) * M;
  double u = -INFINITY, s = 0.0;
  if (live)
    for (int m = qd; m < M; m += 4) u = fmax(u, gf[m]);
  u = fmax(u, __shfl_xor(u, 1));
  u = fmax(u, __shfl_xor(u, 2));
  if (live)
    for (int m = qd; m < M; m += 4) s += exp(gf[m] - u);
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  const double lse = live ? u + log(s) : 0.0;
  if (live)
    for (int m = qd; m < M; m += 4) gf[m] = exp(gf[m] - lse);
  double ll = (qd == 0) ? lse : 0.0;
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) ll += __shfl_xor(ll, sh);
  if (lane == 0 && wave < 4) red[wave] = ll;
  __syncthreads();
  if (tid == 0) llpart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// PHASE 2.  Workgroup (segment of kBdSeg frames, block of 16 pairs); its four waves take the 16-mixture tiles in turn.
// Per k-step of four frames: A = gamma[frame][mixture], B = x, y, x^2, y^2, x y of the 16 pairs -> five accumulators
//   acc[r] of lane (lgrp, lcol) = S[mixture 16 tile + lgrp + 4 r][pair 16 pb + lcol]      (the f64 C/D layout).
// A k-step whose 64 responsibilities are all exactly 0 adds exactly nothing and is skipped (wave-uniform).  Row `seg` of
// `part` has the layout of the statistics; every element of it is written by exactly one lane of one workgroup.
__global__ void __launch_bounds__(256)
estep_bdiag_stats_kernel(const double *__restrict__ X, int64_t n0, int64_t nfr, int Dj, int M, const double *__restrict__ G,
                         double *__restrict__ part, int64_t plen) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lcol = lane & 15, lgrp = lane >> 4, D = Dj / 2;
  const int seg = blockIdx.x, pb = blockIdx.y;
  const int64_t fb = (int64_t)seg * kBdSeg, fe = (fb + kBdSeg < nfr) ? fb + kBdSeg : nfr;
  const int d = 16 * pb + lcol;
  const bool dl = d < D;
  double *P = part + (size_t)seg * plen;
  if (pb == 0 && tid == 0) P[plen - 1] = 0.0;          // (the log-likelihood is summed from phase 1's partials)
  const int ntile = (M + 15) / 16;
  for (int tile = wave; tile < ntile; tile += 4) {
    d4 ax = {0, 0, 0, 0}, ay = {0, 0, 0, 0}, axx = {0, 0, 0, 0}, ayy = {0, 0, 0, 0}, axy = {0, 0, 0, 0};
    double s0l = 0.0;
    const int mc = 16 * tile + lcol;
    const bool ml = mc < M;
    for (int64_t k = fb; k < fe; k += 16) {            // four k-steps: their gamma loads are in flight together
      double gv[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int64_t f = k + 4 * t + lgrp;
        gv[t] = (ml && f < fe) ? G[(size_t)f * M + mc] : 0.0;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double gm = gv[t];
        if (__builtin_amdgcn_ballot_w64(gm != 0.0) == 0) continue;
        const int64_t f = k + 4 * t + lgrp;
        double x = 0.0, y = 0.0;
        if (dl && f < fe) {
          const double *xr = X + (size_t)(n0 + f) * Dj;
          x = xr[d];
          y = xr[D + d];
        }
        ax = __builtin_amdgcn_mfma_f64_16x16x4f64(gm, x, ax, 0, 0, 0);
        ay = __builtin_amdgcn_mfma_f64_16x16x4f64(gm, y, ay, 0, 0, 0);
        axx = __builtin_amdgcn_mfma_f64_16x16x4f64(gm, x * x, axx, 0, 0, 0);
        ayy = __builtin_amdgcn_mfma_f64_16x16x4f64(gm, y * y, ayy, 0, 0, 0);
        axy = __builtin_amdgcn_mfma_f64_16x16x4f64(gm, x * y, axy, 0, 0, 0);
        s0l += gm;
      }
    }
    if (pb == 0) {
      s0l += __shfl_xor(s0l, 16);
      s0l += __shfl_xor(s0l, 32);
      if (lgrp == 0 && ml) P[mc] = s0l;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 16 * tile + 4 * r + lgrp;
      if (m < M && dl) {
        double *s1 = P + M + (size_t)m * Dj, *s2 = P + M + (size_t)M * Dj + (size_t)m * Dj;
        s1[d] = ax[r];
        s1[D + d] = ay[r];
        s2[d] = axx[r];
        s2[D + d] = ayy[r];
        P[M + 2 * (size_t)M * Dj + (size_t)m * D + d] = axy[r];
      }
    }
  }
}

struct EstepBdiagScratch {
  DevBuf<double> raw, prm, cst, G, llpart, part;
  DevBuf<int> flag;
  StreamOrder order;     // calls of one thread on different streams share the buffers above
};
static EstepBdiagScratch &bdiag_scratch() {
  static thread_local EstepBdiagScratch s;
  return s;
}

int estep_bdiag_check_dims(const char *who, int Dj, int M) {
  if (Dj < 2 || (Dj & 1) || M < 1) return fail(VCMI_ERR_DIM, "%s: Dj=%d M=%d invalid (the joint dimension must be even)", who, Dj, M);
  if (Dj > kBdiagMaxDj) return fail(VCMI_ERR_DIM, "%s: joint dimension %d exceeds the block-diagonal E-step limit (%d)", who, Dj, kBdiagMaxDj);
  if (M > kBdiagMaxM) return fail(VCMI_ERR_DIM, "%s: %d mixtures exceed the block-diagonal E-step limit (%d)", who, M, kBdiagMaxM);
  return VCMI_OK;
}

// the kernels of one E-step under the DEVICE parameter block draw; sc is entered (StreamOrderScope) by the caller
static int estep_bdiag_run(EstepBdiagScratch &sc, const double *dX, int64_t N, int Dj, int M, const double *draw, int *dflag,
                           double *dstats, hipStream_t st) {
  const int D = Dj / 2;
  const int64_t plen = vcmi_estep_bdiag_stats_len(Dj, M);
  const int64_t chunk = N < kBdChunk ? N : kBdChunk;
  const int rows = (int)((chunk + kBdSeg - 1) / kBdSeg), blocks = (int)((chunk + kBdFB - 1) / kBdFB);
  VCMI_TRY(sc.prm.reserve((size_t)M * D * kBdPrm));
  VCMI_TRY(sc.cst.reserve(M));
  VCMI_TRY(sc.G.reserve((size_t)chunk * M));
  VCMI_TRY(sc.llpart.reserve(blocks));
  VCMI_TRY(sc.part.reserve((size_t)rows * plen));
  const size_t lds = (size_t)Dj * kBdRS * sizeof(double);       // 133 KB at Dj = 256, of the 160 KB of a CU
  static std::atomic<bool> attr_done[64];
  VCMI_TRY(set_max_dynamic_lds(estep_bdiag_gamma_kernel, (size_t)kBdiagMaxDj * kBdRS * sizeof(double), attr_done));
  hipLaunchKernelGGL(estep_bdiag_prep_kernel, dim3(M), dim3(128), 0, st, draw, Dj, M, sc.prm.p, sc.cst.p, dflag);
  VCMI_HIP(hipGetLastError());
  for (int64_t n0 = 0; n0 < N; n0 += kBdChunk) {
    const int64_t nfr = (N - n0 < kBdChunk) ? N - n0 : kBdChunk;
    const int nb = (int)((nfr + kBdFB - 1) / kBdFB), nr = (int)((nfr + kBdSeg - 1) / kBdSeg);
    hipLaunchKernelGGL(estep_bdiag_gamma_kernel, dim3(nb), dim3(kBdGammaThreads), lds, st, dX, n0, nfr, Dj, M, sc.prm.p, sc.cst.p, sc.G.p,
                       sc.llpart.p);
    VCMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(estep_bdiag_stats_kernel, dim3(nr, (D + 15) / 16), dim3(256), 0, st, dX, n0, nfr, Dj, M, sc.G.p, sc.part.p, plen);
    VCMI_HIP(hipGetLastError());
    estep_reduce_launch(sc.part.p, nr, plen, dstats, st, /*accumulate=*/n0 > 0);
    estep_sum_launch(sc.llpart.p, nb, dstats + (plen - 1), st);
    VCMI_HIP(hipGetLastError());
  }
  return VCMI_OK;
}

int estep_bdiag_device_block(const double *dX, int64_t N, int Dj, int M, const double *dparams, int *dflag, double *dstats,
                             hipStream_t st) {
  if (N == 0) {
    VCMI_HIP(hipMemsetAsync(dstats, 0, sizeof(double) * (size_t)vcmi_estep_bdiag_stats_len(Dj, M), st));
    return VCMI_OK;
  }
  EstepBdiagScratch &sc = bdiag_scratch();
  StreamOrderScope use(sc.order, st);
  VCMI_TRY(use.status());
  return estep_bdiag_run(sc, dX, N, Dj, M, dparams, dflag, dstats, st);
}

}  // namespace vcmi

using namespace vcmi;

extern "C" int64_t vcmi_estep_bdiag_stats_len(int Dj, int M) { return (int64_t)M * (1 + 2 * (int64_t)Dj + Dj / 2) + 1; }

extern "C" int vcmi_estep_bdiag_dev(const double *dX, int64_t N, int Dj, int M, const double *w, const double *mu,
                                    const double *covars, double *dstats, void *stream) {
  if (N < 0) return fail(VCMI_ERR_DIM, "vcmi_estep_bdiag_dev: N=%lld invalid", (long long)N);
  VCMI_TRY(estep_bdiag_check_dims("vcmi_estep_bdiag_dev", Dj, M));
  if (!w || !mu || !covars || !dstats || (N > 0 && !dX)) return fail(VCMI_ERR_ARG, "vcmi_estep_bdiag_dev: NULL argument");
  hipStream_t st = as_stream(stream);
  if (N == 0) return estep_bdiag_device_block(dX, 0, Dj, M, nullptr, nullptr, dstats, st);
  EstepBdiagScratch &sc = bdiag_scratch();
  int bad = INT_MAX;
  {   // the parameter staging is rewritten before the kernels run; the host waits outside the scope
    StreamOrderScope use(sc.order, st);
    VCMI_TRY(use.status());
    const size_t md = (size_t)M * Dj, mc = (size_t)M * (Dj + Dj / 2);
    VCMI_TRY(sc.raw.reserve(M + md + mc));
    VCMI_TRY(sc.flag.reserve(1));
    VCMI_TRY(staged_upload(sc.raw.p, w, sizeof(double) * M, st));
    VCMI_TRY(staged_upload(sc.raw.p + M, mu, sizeof(double) * md, st));
    VCMI_TRY(staged_upload(sc.raw.p + M + md, covars, sizeof(double) * mc, st));
    VCMI_TRY(staged_upload(sc.flag.p, &bad, sizeof(int), st));
    VCMI_TRY(estep_bdiag_run(sc, dX, N, Dj, M, sc.raw.p, sc.flag.p, dstats, st));
    VCMI_HIP(hipMemcpyAsync(&bad, sc.flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  }
  VCMI_HIP(hipStreamSynchronize(st));
  if (bad != INT_MAX) {
    const int D = Dj / 2;
    return fail(VCMI_ERR_NOT_PD, "vcmi_estep_bdiag_dev: pair (%d,%d) is not positive definite", (bad - 1) % D + 1, (bad - 1) / D + 1);
  }
  return VCMI_OK;
}
