// traj_gvd_plan.hpp -- the launch rule of traj_gvd_kernel (traj_gv_diag.hip) and the workspace arithmetic of a GV call over
// diagonal conditional precisions.  HOST arithmetic only, no HIP: tests/c/traj_gvd_plan_check.cpp compiles it alone, and
// tests/gv_diag_restatement.py restates it (gvd_resident).
#pragma once
#include <cstddef>
#include <cstdint>

namespace vcmi {

static constexpr int kGvdThreads = 512;                 // 8 waves, two per SIMD; thread = (static dimension, frame phase): D <= 512
static constexpr size_t kGvdLdsLimit = 160 * 1024 - 256;   // what a workgroup may ask of the CU's 160 KB

// The ascent works on five (T,D) arrays per utterance: y, the second y of the Jacobi step, c2 = P[t,t-2], c0 = P[t,t], r.
static constexpr int kGvdArrays = 5;

// LDS of the kernel without any of them: the two reduction rows and mean, var, coef
inline size_t gvd_fixed_lds_bytes(int D) { return (2 * (size_t)kGvdThreads + 3 * (size_t)D) * sizeof(double); }

// How many of the five arrays stay in LDS across the epochs, from the static dimension and the LONGEST utterance of the call:
// as many as fit, in the order above; 0 when not even the two y do (one y alone in LDS would leave the Jacobi step with one
// operand in each memory for nothing).  The rest is streamed from the workspace (and Y).
inline int gvd_resident(int D, int64_t Tmax) {
  const size_t one = (size_t)Tmax * (size_t)D * sizeof(double), fixed = gvd_fixed_lds_bytes(D);
  if (one == 0 || fixed >= kGvdLdsLimit) return 0;
  const size_t fit = (kGvdLdsLimit - fixed) / one;
  return fit >= (size_t)kGvdArrays ? kGvdArrays : (fit >= 2 ? (int)fit : 0);
}
inline size_t gvd_lds_bytes(int D, int64_t Tmax) {
  return gvd_fixed_lds_bytes(D) + (size_t)gvd_resident(D, Tmax) * (size_t)Tmax * (size_t)D * sizeof(double);
}

// Workspace of a call in diagonal mode, in doubles: the solver's (nframes,D) and, with GV, four more of them (second y, c2, c0, r)
// behind it, every one indexed by the utterance's frame0.
inline int64_t gvd_ws_doubles(int64_t nframes, int D, bool with_gv) { return nframes * D * (with_gv ? kGvdArrays : 1); }

}  // namespace vcmi
