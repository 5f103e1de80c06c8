// estep_generic.hpp -- the kernels of the diagonal E-step that are no MFMA kernels (included by estep.hip): the generic path for
// any (Dj, M) -- responsibilities to an HBM workspace in chunks of kChunk frames, per-(m,d) sequential accumulation over
// segments of kSeg frames -- the fixed-order reduction and sum every path ends in, the combination of groups of 128 mixtures
// (M > 128), and the padding of an odd joint dimension.  kChunk, kSeg: estep_cfg.hpp.
#pragma once
#include "estep_cfg.hpp"

namespace vcmi {

// one lane per frame: responsibilities gamma (chunk-local (n,M) row-major) and lse
__global__ void __launch_bounds__(64)
estep_gamma_kernel(const double *__restrict__ X, int64_t n0, int64_t nfr, int Dj, int M, const double *__restrict__ mu,
                   const double *__restrict__ iv, const double *__restrict__ cst, double *__restrict__ G,
                   double *__restrict__ LSE) {
  extern __shared__ double xs[];   // [Dj][64]
  const int lane = threadIdx.x;
  const int64_t nl = (int64_t)blockIdx.x * 64 + lane;
  const bool live = nl < nfr;
  for (int d = 0; d < Dj; ++d) xs[d * 64 + lane] = live ? X[(n0 + nl) * Dj + d] : 0.0;
  double *g = G + nl * M;
  double u = -INFINITY;
  for (int m = 0; m < M; ++m) {
    double q = 0.0;
    for (int d = 0; d < Dj; ++d) {
      const double df = xs[d * 64 + lane] - mu[(size_t)m * Dj + d];
      q = fma(df * df, iv[(size_t)m * Dj + d], q);
    }
    const double l = cst[m] - 0.5 * q;
    if (live) g[m] = l;
    u = fmax(u, l);
  }
  if (!live) return;
  double s = 0.0;
  for (int m = 0; m < M; ++m) s += exp(g[m] - u);
  const double lse = u + log(s);
  for (int m = 0; m < M; ++m) g[m] = exp(g[m] - lse);
  LSE[nl] = lse;
}

// thread per statistic element e = m*Dj + d, sequential over the frames of one segment
__global__ void __launch_bounds__(256)
estep_stats_kernel(const double *__restrict__ X, int64_t n0, int64_t nfr, int Dj, int M, const double *__restrict__ G,
                   const double *__restrict__ LSE, double *__restrict__ part, int64_t plen) {
  const int seg = blockIdx.x;
  const int e = blockIdx.y * 256 + threadIdx.x;
  const int64_t f0 = (int64_t)seg * kSeg, f1 = (f0 + kSeg < nfr) ? f0 + kSeg : nfr;
  double *P = part + (size_t)seg * plen;
  if (e < M * Dj) {
    const int m = e / Dj, d = e % Dj;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t f = f0; f < f1; ++f) {
      const double g = G[f * M + m], x = X[(n0 + f) * Dj + d];
      s0 += g;
      s1 = fma(g, x, s1);
      s2 = fma(g * x, x, s2);
    }
    if (d == 0) P[m] = s0;
    P[M + e] = s1;
    P[M + (size_t)M * Dj + e] = s2;
  }
  if (e == 0) {
    double ll = 0.0;
    for (int64_t f = f0; f < f1; ++f) ll += LSE[f];
    P[plen - 1] = ll;
  }
}

// stats[e] (+)= sum over the partial rows (accumulate = 0: stats need no memset before), in a FIXED order (deterministic): four threads per element each add up every
// fourth row in increasing order, then ((p0 + p1) + (p2 + p3)).  (One thread per element walking all rows one after the
// other left two thirds of the CUs idle and took 64 us for the 256 rows of the benchmark E-step -- 4 % of the step.)
__global__ void __launch_bounds__(256)
estep_reduce_kernel(const double *__restrict__ part, int nrows, int64_t plen, double *__restrict__ stats, int accumulate,
                    const int64_t *__restrict__ only_if) {
  if (only_if && *only_if == 0) return;      // (the soft frames of estep_hard.hpp: without any, the partials were not written)
  __shared__ double psum[4][64];
  const int el = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int64_t e = (int64_t)blockIdx.x * 64 + el;
  double s = 0.0;
  if (e < plen) {
    const double *p = part + e;
    int r = q;
    for (; r + 28 < nrows; r += 32) {              // eight independent loads in flight, added in row order
      const double v0 = p[(size_t)r * plen], v1 = p[(size_t)(r + 4) * plen], v2 = p[(size_t)(r + 8) * plen], v3 = p[(size_t)(r + 12) * plen],
                   v4 = p[(size_t)(r + 16) * plen], v5 = p[(size_t)(r + 20) * plen], v6 = p[(size_t)(r + 24) * plen], v7 = p[(size_t)(r + 28) * plen];
      s += v0; s += v1; s += v2; s += v3; s += v4; s += v5; s += v6; s += v7;
    }
    for (; r < nrows; r += 4) s += p[(size_t)r * plen];
  }
  psum[q][el] = s;
  __syncthreads();
  if (q == 0 && e < plen) stats[e] = (accumulate ? stats[e] : 0.0) + ((psum[0][el] + psum[1][el]) + (psum[2][el] + psum[3][el]));
}

// More than 128 mixtures (groups of 128, one PHASE 3 launch each): the responsibilities G_g[f][.] are normalised within
// group g and lse_g[f] is the group's log-sum-exp.  Here, per frame: L = log sum_g e^(lse_g) (max-shifted, groups in
// order), G_g[f][.] *= e^(lse_g - L), and the frame's L goes into a per-workgroup partial of the log-likelihood (summed
// in fixed order by estep_sum_kernel).  One wave per frame; G is [group][n][128], lse [group][n].
__global__ void __launch_bounds__(256)
estep_group_combine_kernel(double *__restrict__ G, const double *__restrict__ lse, int ngroups, int64_t n, int64_t gstride,
                           double *__restrict__ llpart) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  for (int64_t f = (int64_t)blockIdx.x * 4 + wave; f < n; f += (int64_t)gridDim.x * 4) {
    double u = -INFINITY;
    for (int g = 0; g < ngroups; ++g) u = fmax(u, lse[(size_t)g * n + f]);
    double s = 0.0;
    for (int g = 0; g < ngroups; ++g) s += exp(lse[(size_t)g * n + f] - u);
    const double L = u + log(s);
    for (int g = 0; g < ngroups; ++g) {
      const double lg = lse[(size_t)g * n + f];
      double *row = G + (size_t)g * gstride + f * 128;
      if (lg == -INFINITY) {                    // a group without any weight: its responsibilities are exactly zero
        row[lane] = 0.0;
        row[lane + 64] = 0.0;
        continue;
      }
      const double sc = exp(lg - L);
      row[lane] *= sc;
      row[lane + 64] *= sc;
    }
    acc += L;                                   // (every lane holds the same value)
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) llpart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// partial statistics of one mixture group (rows of plen_g = Mg (1 + 2 dj) + 1 doubles: [S0 | S1 (dj,Mg) | S2 (dj,Mg) | unused])
// summed in row order and added into the full layout at mixture m0
__global__ void __launch_bounds__(256)
estep_group_reduce_kernel(const double *__restrict__ part, int nrows, int64_t plen_g, int Mg, int dj, int m0, int M,
                          double *__restrict__ stats) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, per = (int64_t)Mg * dj;
  if (e >= plen_g - 1) return;
  double s = 0.0;
  for (int r = 0; r < nrows; ++r) s += part[(size_t)r * plen_g + e];
  const int64_t dst = e < Mg ? m0 + e : e < Mg + per ? M + (int64_t)m0 * dj + (e - Mg) : M + (int64_t)M * dj + (int64_t)m0 * dj + (e - Mg - per);
  stats[dst] += s;
}

// deterministic sum of n doubles into out[0] (+=): one workgroup, strided partials then a sequential tail
__global__ void __launch_bounds__(256)
estep_sum_kernel(const double *__restrict__ v, int64_t n, double *__restrict__ out) {
  __shared__ double part[256];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += v[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = out[0];
    for (int i = 0; i < 256; ++i) t += part[i];
    out[0] = t;
  }
}

// Odd joint dimension: the MFMA kernels stream X by 16-byte LDS-DMA rows, i.e. need an even row length.  The frames are
// copied with one extra dimension that is identically 0 under a unit-variance, zero-mean parameter: it adds
// (0 - 0)^2 / 1 = 0 to every distance and log 1 = 0 to every log-determinant -- the statistics of the real dimensions are
// those of the unpadded problem; its own statistics are dropped again and the extra -log(2 pi)/2 per frame is added back.
__global__ void __launch_bounds__(256)
estep_pad_x_kernel(const double *__restrict__ X, int64_t n, int dj, double *__restrict__ Xp) {
  const int djp = dj + 1;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n * djp; e += (int64_t)gridDim.x * 256) {
    const int64_t f = e / djp;
    const int d = (int)(e - f * djp);
    Xp[e] = d < dj ? X[f * dj + d] : 0.0;
  }
}
// stats_p ([S0 (M) | S1 (dj+1,M) | S2 (dj+1,M) | ll]) added into stats ([S0 | S1 (dj,M) | S2 (dj,M) | ll])
__global__ void __launch_bounds__(256)
estep_unpad_stats_kernel(const double *__restrict__ sp, int M, int dj, int64_t nframes, double *__restrict__ stats) {
  const int djp = dj + 1;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, per = (int64_t)M * dj;
  if (e < M) stats[e] += sp[e];
  if (e < per) {
    const int64_t m = e / dj, d = e - m * dj;
    stats[M + e] += sp[M + m * djp + d];
    stats[M + per + e] += sp[M + (int64_t)M * djp + m * djp + d];
  }
  // the padding dimension put one more -log(2 pi)/2 into every frame's log-density
  if (e == 0) stats[M + 2 * per] += sp[M + 2 * (int64_t)M * djp] + (double)nframes * (0.5 * kLog2Pi);
}

}  // namespace vcmi
