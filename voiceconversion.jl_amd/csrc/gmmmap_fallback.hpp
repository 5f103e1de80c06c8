// gmmmap_fallback.hpp -- the host launch functions of gmmmap_fallback.hip, called by the device routines of gmmmap.hip.  (The
// library is built without relocatable device code: a kernel is launched by a host function of the file that defines it.)
#pragma once
#include "vcmi_common.hpp"

struct vcmi_gmmmap;

namespace vcmi {
// gmmmap_generic_kernel<mode>: 0 convert (dY (T, ldy)), 1 log-weighted densities (dY = LP (T,M), ldy = M)
int gmmmap_generic_launch(const vcmi_gmmmap *g, int mode, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy,
                          hipStream_t st);
// logdens_tiled_kernel: log-weighted densities (T,M) for 16 < D <= 160 from the generic layout
int logdens_tiled_launch(const vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dLP, hipStream_t st);
// posterior_finish_kernel<mode> on (T,M) log-weighted densities: 0 posterior in place, 1 the 1-based argmax into didx
int posterior_finish_launch(int mode, double *dLP, int M, int64_t T, int64_t *didx, hipStream_t st);
// convert_from_logdens_kernel: y of T frames from their log-weighted densities dLP (T,M) and the transposed regression g->At
int convert_from_logdens_launch(const vcmi_gmmmap *g, const double *dLP, const double *dX, int64_t ldx, int64_t T, double *dY,
                                int64_t ldy, hipStream_t st);
}  // namespace vcmi
