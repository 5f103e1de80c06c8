// traj_gvp_plan.hpp -- the launch rule of traj_gvp_kernel (traj_gv_penta.hip) and the workspace arithmetic of a GV call over a
// converter with THREE windows (vcmi_trajgv_create_bdiag over a handle of vcmi_traj_create_bdiag_windows(b, T, 3)).  HOST
// arithmetic only, no HIP: tests/c/traj_gvp_check.cpp compiles it alone, and tests/gv_penta_restatement.py restates it
// (gvp_resident).  traj_penta_plan.hpp keeps the rule of a call without GV, unchanged.
#pragma once
#include <cstddef>
#include <cstdint>

#include "traj_penta_plan.hpp"

namespace vcmi {

// The ascent works on six (T,D) arrays per utterance, in the order in which they take LDS: y and the second y of the Jacobi step
// (an epoch reads five y per element), c1 = P[t-1,t] and c2 = P[t-2,t] (read twice per element: their own and the one of frame
// t+1 / t+2), then c0 = P[t,t] and r (read once).
static constexpr int kGvpArrays = 6;

// LDS of the kernel without any of them: traj_gvd_kernel's (the two reduction rows and mean, var, coef), 512 threads as there
inline size_t gvp_fixed_lds_bytes(int D) { return gvd_fixed_lds_bytes(D); }

// How many of the six stay in LDS across the epochs, from the static dimension and the LONGEST utterance of the call: as many
// as fit kGvdLdsLimit, in the order above; 0 when not even the two y do.  The rest is streamed from the workspace (and Y).
inline int gvp_resident(int D, int64_t Tmax) {
  const size_t one = (size_t)Tmax * (size_t)D * sizeof(double), fixed = gvp_fixed_lds_bytes(D);
  if (one == 0 || fixed >= kGvdLdsLimit) return 0;
  const size_t fit = (kGvdLdsLimit - fixed) / one;
  return fit >= (size_t)kGvpArrays ? kGvpArrays : (fit >= 2 ? (int)fit : 0);
}
inline size_t gvp_lds_bytes(int D, int64_t Tmax) {
  return gvp_fixed_lds_bytes(D) + (size_t)gvp_resident(D, Tmax) * (size_t)Tmax * (size_t)D * sizeof(double);
}

// Workspace of a three-window call, in doubles.  Without GV: the solver's l1 and l2 (penta_ws_doubles).  With GV: five
// (nframes,D) arrays indexed by the utterance's frame0 -- the second y, c1, c2, c0, r (the first y is the utterance's Y).  l1 and
// l2 are dead once the solve has run on the stream, and the ascent runs behind it on the same stream: the second y lies ON l1
// and c1 ON l2, so a GV call asks for five arrays, not seven.
static constexpr int kGvpWsArrays = kGvpArrays - 1;
inline int64_t gvp_ws_offset(int k, int64_t nframes, int D) { return (int64_t)k * nframes * D; }     // k: 0 second y, 1 c1, 2 c2, 3 c0, 4 r
inline int64_t gvp_ws_doubles(int64_t nframes, int D, bool with_gv) {
  return with_gv ? kGvpWsArrays * nframes * D : penta_ws_doubles(nframes, D);
}

}  // namespace vcmi
