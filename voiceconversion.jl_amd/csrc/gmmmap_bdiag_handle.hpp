// gmmmap_bdiag_handle.hpp -- the vcmi_bdmap handle and what trajectory conversion straight from it (traj.hip, traj_diag.hip:
// vcmi_traj_create_bdiag) calls in gmmmap_bdiag.hip.  HOST functions only: a kernel is launched by the file that defines it.
#pragma once
#include "vcmi_common.hpp"

// The handle converts on the device it was created on: device groups (vcmi_set_devices) do not shard its calls.
struct vcmi_bdmap {
  int D = 0, DP = 0, M = 0, device = 0;
  int FB = 64;                        // frames per workgroup
  vcmi::DevBuf<double> prm1, prm3, cst;      // BdmapTable's, resident
  vcmi::DevBuf<double> prm4;          // ... and the trajectory table [M][DP][mu_x, a, mu_y, q]
  std::vector<double> h_a;            // (D,M)
  std::vector<double> h_q;            // (D,M) reciprocal conditional variances: the solver's table of a trajectory converter
  int64_t q_bad = -1;                 // BdmapTable::q_bad
};

namespace vcmi {

// The fused arg-max + g_t pass of a trajectory converter made from the handle: dense frames X (T, dim), mhat (T) 1-based first
// maximum of the log-density, G (T, dim) = q_mhat (.) (mu_y + a (x - mu_x)).  Asynchronous on st; VCMI_ERR_ARG from another
// device than the handle's.
int bdmap_traj_device(const vcmi_bdmap *h, const double *dX, int64_t T, int64_t *mhat, double *G, hipStream_t st);

}  // namespace vcmi
