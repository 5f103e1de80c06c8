// bdiag_pair.hpp -- the 2 x 2 block [vx c; c vy] of one pair of a cross-diagonal ("block_diag") model: its determinant and
// the validity test, for host and device code.  No HIP header: the host-only preparation files (gmmmap_bdiag_prepare.cpp)
// and their stand-alone checks include it with a plain C++ compiler.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VCMI_HOST_DEVICE __host__ __device__
#else
#define VCMI_HOST_DEVICE
#endif

namespace vcmi {

// vx vy - c^2 to a few ulps also where it cancels (Kahan's 2 x 2 determinant: the rounding of c c is added back)
VCMI_HOST_DEVICE inline double bdiag_det(double vx, double vy, double c) {
  const double cc = c * c;
  return fma(vx, vy, -cc) - fma(c, c, -cc);
}
// the pair's 2 x 2 block is positive definite (a NaN anywhere: not)
VCMI_HOST_DEVICE inline bool bdiag_pair_valid(double vx, double vy, double c) {
  return vx > 0.0 && vy > 0.0 && bdiag_det(vx, vy, c) > 0.0;
}
// index d + D m of the first pair of covars (Dj + D, M) that is not valid, -1: none
inline int64_t first_bad_pair(const double *covars, int Dj, int M) {
  const int D = Dj / 2;
  for (int m = 0; m < M; ++m) {
    const double *cv = covars + (size_t)m * (Dj + D);
    for (int d = 0; d < D; ++d)
      if (!bdiag_pair_valid(cv[d], cv[D + d], cv[Dj + d])) return d + (int64_t)D * m;
  }
  return -1;
}

}  // namespace vcmi
