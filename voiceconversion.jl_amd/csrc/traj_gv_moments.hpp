// traj_gv_moments.hpp -- the two-pass, fixed-order moments of a trajectory, shared by the kernels of the global-variance ascent
// (traj_gv.hip, traj_gv_band.hpp).  Device code, included by the files that launch those kernels.
#pragma once

namespace vcmi {

// mean and corrected variance of every static dimension of y (T,D), by all threads of the workgroup: thread = (dimension
// tid % D, frame group tid / D); red: 2 * nthr doubles of LDS, mean / var: D each.  Ends with a barrier.
template <typename YP>
__device__ void gv_moments(YP y, int D, int T, int nthr, double *red, double *mean, double *var) {
  const int tid = threadIdx.x;
  const int NG = nthr / D;                 // frame groups per dimension
  const int d = tid % D, g = tid / D;
  double s = 0.0;
  if (g < NG) {
    // 8 loads in flight per thread (a plain loop keeps one: with one workgroup per CU the passes of this kernel are
    // bound by memory-level parallelism, not by HBM bandwidth); the additions stay in frame order
    int t = g;
    for (; t + 7 * NG < T; t += 8 * NG) {
      double v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = y[(size_t)(t + q * NG) * D + d];
#pragma unroll
      for (int q = 0; q < 8; ++q) s += v[q];
    }
    for (; t < T; t += NG) s += y[(size_t)t * D + d];
  }
  if (g < NG) red[g * D + d] = s;
  __syncthreads();
  if (tid < D) {
    double m = 0.0;
    for (int k = 0; k < NG; ++k) m += red[k * D + tid];
    mean[tid] = m / (double)T;
  }
  __syncthreads();
  s = 0.0;
  if (g < NG) {
    const double m = mean[d];
    int t = g;
    for (; t + 7 * NG < T; t += 8 * NG) {
      double v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = y[(size_t)(t + q * NG) * D + d];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const double e = v[q] - m;
        s = fma(e, e, s);
      }
    }
    for (; t < T; t += NG) {
      const double e = y[(size_t)t * D + d] - m;
      s = fma(e, e, s);
    }
    red[g * D + d] = s;
  }
  __syncthreads();
  if (tid < D) {
    double v = 0.0;
    for (int k = 0; k < NG; ++k) v += red[k * D + tid];
    var[tid] = v / (double)(T - 1);        // Julia's var: corrected
  }
  __syncthreads();
}

}  // namespace vcmi
