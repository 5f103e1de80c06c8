// traj_band_plan.hpp -- the launch rules and the workspace arithmetic of the BAND family: trajectory conversion over diagonal
// conditional precisions, with two windows (static + delta: traj_diag.hip) or three (+ delta-delta: traj_penta.hip), and the GV
// ascent behind either solve (traj_gv_band.hip: traj_gvd_kernel, traj_gvp_kernel).  HOST arithmetic only, no HIP:
// tests/c/traj_gvd_plan_check.cpp, traj_gvp_check.cpp and traj_penta_check.cpp compile it alone, and tests/gv_diag_restatement.py /
// gv_penta_restatement.py restate the residency rule.
#pragma once
#include <cstddef>
#include <cstdint>

namespace vcmi {

// ---- the solvers ----
// Workspace of a solve, (nframes,D) arrays indexed by the utterance's frame0: the tridiagonal solver's u; the pentadiagonal
// solver's l1 (where u is) and l2 behind it.
static constexpr int kPentaArrays = 2;
inline int band_solver_arrays(int windows) { return windows == 3 ? kPentaArrays : 1; }
inline int64_t penta_l1_offset(int64_t, int) { return 0; }
inline int64_t penta_l2_offset(int64_t nframes, int D) { return nframes * D; }
// the pentadiagonal solver: one wave per (utterance, slab of static dimensions), lane = dimension
static constexpr int kPentaSlab = 64;
inline int penta_slabs(int D) { return (D + kPentaSlab - 1) / kPentaSlab; }

// ---- the GV ascents ----
static constexpr int kGvdThreads = 512;                 // 8 waves, two per SIMD; thread = (static dimension, frame phase): D <= 512
static constexpr size_t kGvdLdsLimit = 160 * 1024 - 256;   // what a workgroup may ask of the CU's 160 KB

// An ascent works on (T,D) arrays per utterance, in the order in which they take LDS and the workspace: y and the second y of
// the Jacobi step, then the columns of P that an epoch reads twice per element, then those it reads once.
//   two windows:    y, second y,     c2 = P[t-2,t], c0 = P[t,t], r
//   three windows:  y, second y, c1 = P[t-1,t], c2,            c0, r
static constexpr int kGvdArrays = 5, kGvpArrays = 6;
inline int band_gv_arrays(int windows) { return windows == 3 ? kGvpArrays : kGvdArrays; }

// LDS of the kernel without any of them: the two reduction rows and mean, var, coef
inline size_t band_fixed_lds_bytes(int D) { return (2 * (size_t)kGvdThreads + 3 * (size_t)D) * sizeof(double); }

// How many of the `arrays` stay in LDS across the epochs, from the static dimension and the LONGEST utterance of the call: as
// many as fit, in the order above; 0 when not even the two y do (one y alone in LDS would leave the Jacobi step with one operand
// in each memory for nothing).  The rest is streamed from the workspace (and Y).
inline int band_resident(int arrays, int D, int64_t Tmax) {
  const size_t one = (size_t)Tmax * (size_t)D * sizeof(double), fixed = band_fixed_lds_bytes(D);
  if (one == 0 || fixed >= kGvdLdsLimit) return 0;
  const size_t fit = (kGvdLdsLimit - fixed) / one;
  return fit >= (size_t)arrays ? arrays : (fit >= 2 ? (int)fit : 0);
}
inline size_t band_lds_bytes(int arrays, int D, int64_t Tmax) {
  return band_fixed_lds_bytes(D) + (size_t)band_resident(arrays, D, Tmax) * (size_t)Tmax * (size_t)D * sizeof(double);
}

// Array k >= 1 of an ascent (the first y is the utterance's Y) in the workspace of its call.  Two windows: the four arrays lie
// behind the solver's u.  Three windows: l1 and l2 are dead once the solve has run on the stream, and the ascent runs behind it
// on the same stream, so the second y lies ON l1 and c1 ON l2.
inline int64_t band_gv_ws_offset(int windows, int k, int64_t nframes, int D) { return (int64_t)(windows == 3 ? k - 1 : k) * nframes * D; }

// Workspace of a call, in doubles: the solver's arrays; with GV, what the last array of the ascent ends at (five arrays either way).
inline int64_t band_ws_doubles(int windows, int64_t nframes, int D, bool with_gv) {
  return with_gv ? band_gv_ws_offset(windows, band_gv_arrays(windows), nframes, D) : band_solver_arrays(windows) * nframes * D;
}

// ---- the names the checks under tests/c assert by ----
inline size_t gvd_fixed_lds_bytes(int D) { return band_fixed_lds_bytes(D); }
inline size_t gvp_fixed_lds_bytes(int D) { return band_fixed_lds_bytes(D); }
inline int gvd_resident(int D, int64_t Tmax) { return band_resident(kGvdArrays, D, Tmax); }
inline int gvp_resident(int D, int64_t Tmax) { return band_resident(kGvpArrays, D, Tmax); }
inline size_t gvd_lds_bytes(int D, int64_t Tmax) { return band_lds_bytes(kGvdArrays, D, Tmax); }
inline size_t gvp_lds_bytes(int D, int64_t Tmax) { return band_lds_bytes(kGvpArrays, D, Tmax); }
static constexpr int kGvpWsArrays = kGvpArrays - 1;
inline int64_t gvp_ws_offset(int k, int64_t nframes, int D) { return band_gv_ws_offset(3, k + 1, nframes, D); }     // k: 0 second y .. 4 r
inline int64_t penta_ws_doubles(int64_t nframes, int D) { return band_ws_doubles(3, nframes, D, false); }
inline int64_t gvd_ws_doubles(int64_t nframes, int D, bool with_gv) { return band_ws_doubles(2, nframes, D, with_gv); }
inline int64_t gvp_ws_doubles(int64_t nframes, int D, bool with_gv) { return band_ws_doubles(3, nframes, D, with_gv); }
// the SOLVER's share of a call: three windows keep l1 and l2 whether or not an ascent follows
inline int64_t traj_diag_ws_doubles(int windows, int64_t nframes, int D, bool with_gv) {
  return band_ws_doubles(windows, nframes, D, with_gv && windows != 3);
}

}  // namespace vcmi
