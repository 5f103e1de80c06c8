// postf.hpp -- the pre / post steps of vc on DEVICE-RESIDENT matrices: push_delta (src/datasets.jl:6-13)
// and the VarianceScaling post-filter (src/gv.jl:10-15), shared by postf.hip (C entries) and traj_vc.cpp (vc_traj_device, the
// routine behind vcmi_vc_traj_postf / vcmi_vc_traj_static / vcmi_vc_trajgv and their *_dev forms), and the whole-matrix device
// scratch of the host-pointer entries of both files.
#pragma once
#include <functional>
#include "vcmi_common.hpp"

namespace vcmi {
// out (2D,T) with leading dimension ldo  <-  [src; delta(src)], src (D,T) with leading dimension lds; asynchronous on st
int push_delta_device(const double *dsrc, int64_t lds, int D, int64_t T, double *dout, int64_t ldo, hipStream_t st);
// out (3D,T)  <-  [src; delta(src); delta-delta(src)]: the first 2D rows as above, then x_{t-1} - 2 x_t + x_{t+1} with absent neighbours dropped
int push_delta2_device(const double *dsrc, int64_t lds, int D, int64_t T, double *dout, int64_t ldo, hipStream_t st);
// fvpostf!: out[d,t] = sqrt(sigma2[d] / var_d) (src[d,t] - mean_d) + mean_d, mean / corrected variance per row over the T
// frames; sigma2 is a HOST vector (D).  dout may be dsrc (in place).  Asynchronous on st; deterministic (fixed-order sums).
int variance_scaling_device(const double *dsrc, int64_t lds, int D, int64_t T, const double *sigma2_host, double *dout,
                            int64_t ldo, hipStream_t st);
// The statistics half of variance_scaling_device: *dstat receives the per-thread device vector
//   [mean (D) | var (D) | sigma2 (D)], each part kVsStatStride doubles from the previous one,
// for a caller that applies the scale itself (vc_traj_post_device).  It enters the stream order of that vector; the caller
// enqueues its kernel on st and then calls variance_scaling_stats_leave(st).
static constexpr int kVsStatStride = 256;
int variance_scaling_stats_device(const double *dsrc, int64_t lds, int D, int64_t T, const double *sigma2_host,
                                  const double **dstat, hipStream_t st);
int variance_scaling_stats_leave(hipStream_t st);

// The two ends of vc(c::TrajectoryConverter, fm) around the chunk conversions, one streaming pass each.
// pre:  dfm (D+1,T) static features (is_static) or (D2+1,T) -> dx (D2,T) dense, the converter's input; D2 = dim(t): 2D, or 3D
//       for a converter with three windows (never with is_static).  Static input:
//       dx = [fm[2:end,:]; delta] with the delta of push_delta over ALL T frames (bin/vc.jl:77-78).  The power row goes to
//       row 1 of dout (leading dimension ldo) unless dout is NULL (the caller assembles in place in dfm: the row is there).
int vc_traj_pre_device(const double *dfm, int64_t ldf, int D, int D2, int64_t T, bool is_static, double *dx, double *dout, int64_t ldo,
                       hipStream_t st);
// post: dy (D,T) dense -> rows 2..D+1 of dout; with dstat (variance_scaling_stats_device) the rows are scaled on the way.
int vc_traj_post_device(const double *dy, int D, int64_t T, const double *dstat, double *dout, int64_t ldo, hipStream_t st);

// Whole-matrix device scratch of the vc and post-filter entries, one per thread, grow-only between calls: the converter input
// x (2D,T) and result y (D,T) of vc_traj_device under their stream order (the *_dev entries run on the caller's stream), and
// the staging matrix of the host-pointer entries (null stream, every call ends in a blocking download).  A host-pointer entry
// holds a Release for the call: on every way out it waits for the device and frees the three once together they exceed
// kVcScratchKeepBytes, so one long utterance does not keep its footprint for the life of the thread.
static constexpr size_t kVcScratchKeepBytes = (size_t)256 << 20;
// Cap of the precision table [Q_1..Q_M | Qbar of the mixed frames] of the trajectory converter's EM re-estimation (traj_em.hip): a
// batch is processed in slices of whole utterances whose worst case -- every frame mixed -- stays under it (a single longer
// utterance is a slice of its own).  cfg5 (256 x 2000 frames, D = 40: 51 KB per mixed frame, 26 GB in all) runs in two slices.
static constexpr size_t kTrajEmTableCapBytes = (size_t)16 << 30;
struct VcScratch {
  DevBuf<double> x, y, stage;
  StreamOrder order;
  size_t bytes() const { return (x.n + y.n + stage.n) * sizeof(double); }
  struct Release {
    VcScratch &s;
    ~Release() {
      if (s.bytes() <= kVcScratchKeepBytes) return;
      (void)hipDeviceSynchronize();
      s.x.release();
      s.y.release();
      s.stage.release();
    }
  };
};
VcScratch &vc_scratch();   // the calling thread's

// The body of vcmi_vc_frames_batch (vc_batch.hip) for any frame-by-frame converter of dimension D: `convert` turns rows 2..D+1
// of the packed (D+1, N) device matrix (dX, leading dimension ld) into the same rows of the result (dY, same ld), asynchronous
// on st.  Every check, the gather, the per-utterance filter and the scatter are the shared routine's; `who` names the entry in
// its messages.
using FrameConvertFn = std::function<int(const double *dX, int64_t ld, int64_t N, double *dY, hipStream_t st)>;
int vc_frames_batch(int D, const FrameConvertFn &convert, int64_t n, const double *const *fm, const int64_t *T,
                    const double *sigma2, double *const *out, const char *who);
}  // namespace vcmi
