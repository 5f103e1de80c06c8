// traj_penta_plan.hpp -- the launch shape and the workspace arithmetic of the pentadiagonal solver (traj_penta.hip: a converter
// with three windows, vcmi_traj_create_bdiag_windows).  HOST arithmetic only, no HIP: tests/c/traj_penta_check.cpp compiles it
// alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "traj_gvd_plan.hpp"

namespace vcmi {

static constexpr int kPentaSlab = 64;       // static dimensions per wave: lane = dimension
static constexpr int kPentaArrays = 2;      // l1 and l2, (nframes,D) each, indexed by the utterance's frame0

inline int penta_slabs(int D) { return (D + kPentaSlab - 1) / kPentaSlab; }

// l1 lies where the tridiagonal solver has its u, l2 behind it
inline int64_t penta_l1_offset(int64_t, int) { return 0; }
inline int64_t penta_l2_offset(int64_t nframes, int D) { return nframes * D; }
inline int64_t penta_ws_doubles(int64_t nframes, int D) { return kPentaArrays * nframes * D; }

// Workspace of a call over diagonal conditional precisions, in doubles, by the handle's window count: two windows keep
// gvd_ws_doubles (the tridiagonal solver's one array; five with GV), three windows get the two arrays above and nothing else
// (a GV call over such a handle -- vcmi_trajgv_create_bdiag -- does not come through here: traj_gvp_plan.hpp).
inline int64_t traj_diag_ws_doubles(int windows, int64_t nframes, int D, bool with_gv) {
  return windows == 3 ? penta_ws_doubles(nframes, D) : gvd_ws_doubles(nframes, D, with_gv);
}

}  // namespace vcmi
