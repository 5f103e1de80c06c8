// traj_gv_sel.hpp -- where an array of the diagonal-precision GV ascents lives (traj_gv_diag.hip: traj_gvd_kernel;
// traj_gv_penta.hip: traj_gvp_kernel).  Device code, included by the files that define those kernels.
#pragma once
#include "traj_internal.hpp"

namespace vcmi {

// an array of the ascent lives in LDS or in global memory, decided per instantiation: the accesses are ds_ / global_
// instructions, never flat ones
template <bool LDS>
struct GvdPtr {
  typedef gdouble *type;
};
template <>
struct GvdPtr<true> {
  typedef double *type;
};
template <bool LDS>
__device__ __forceinline__ typename GvdPtr<LDS>::type gvd_sel(double *lds, gdouble *glob) {
  if constexpr (LDS) return lds;
  else return glob;
}

}  // namespace vcmi
