// postf.hpp -- the pre / post steps of vc on DEVICE-RESIDENT matrices: push_delta (src/datasets.jl:6-13)
// and the VarianceScaling post-filter (src/gv.jl:10-15), shared by postf.hip (C entries) and traj.hip (vcmi_vc_traj_postf and
// the vcmi_vc_traj_static / vcmi_vc_trajgv / *_dev family).
#pragma once
#include "vcmi_common.hpp"

namespace vcmi {
// out (2D,T) with leading dimension ldo  <-  [src; delta(src)], src (D,T) with leading dimension lds; asynchronous on st
int push_delta_device(const double *dsrc, int64_t lds, int D, int64_t T, double *dout, int64_t ldo, hipStream_t st);
// fvpostf!: out[d,t] = sqrt(sigma2[d] / var_d) (src[d,t] - mean_d) + mean_d, mean / corrected variance per row over the T
// frames; sigma2 is a HOST vector (D).  dout may be dsrc (in place).  Asynchronous on st; deterministic (fixed-order sums).
int variance_scaling_device(const double *dsrc, int64_t lds, int D, int64_t T, const double *sigma2_host, double *dout,
                            int64_t ldo, hipStream_t st);
// The statistics half of variance_scaling_device: *dstat receives the per-thread device vector
//   [mean (D) | var (D) | sigma2 (D)], each part kVsStatStride doubles from the previous one,
// for a caller whose own kernel applies the scale (vc_traj_post_kernel).  It enters the stream order of that vector; the caller
// enqueues its kernel on st and then calls variance_scaling_stats_leave(st).
static constexpr int kVsStatStride = 256;
int variance_scaling_stats_device(const double *dsrc, int64_t lds, int D, int64_t T, const double *sigma2_host,
                                  const double **dstat, hipStream_t st);
int variance_scaling_stats_leave(hipStream_t st);
// rows r0 .. r0 + nrows - 1 of a (ldi, T) matrix -> rows q0 .. of a (ldo, T) matrix (power row / feature rows of vc's matrices)
int copy_rows_device(const double *din, int64_t ldi, int r0, int nrows, int64_t T, double *dout, int64_t ldo, int q0, hipStream_t st);

// The two ends of vc(c::TrajectoryConverter, fm) around the chunk conversions, one streaming pass each.
// pre:  dfm (D+1,T) static features (is_static) or (2D+1,T) -> dx (2D,T) dense, the converter's input.  Static input:
//       dx = [fm[2:end,:]; delta] with the delta of push_delta over ALL T frames (bin/vc.jl:77-78).  The power row goes to
//       row 1 of dout (leading dimension ldo) unless dout is NULL (the caller assembles in place in dfm: the row is there).
int vc_traj_pre_device(const double *dfm, int64_t ldf, int D, int64_t T, bool is_static, double *dx, double *dout, int64_t ldo,
                       hipStream_t st);
// post: dy (D,T) dense -> rows 2..D+1 of dout; with dstat (variance_scaling_stats_device) the rows are scaled on the way.
int vc_traj_post_device(const double *dy, int D, int64_t T, const double *dstat, double *dout, int64_t ldo, hipStream_t st);
}  // namespace vcmi
