// postf.hip -- SURVEY 8(f) rank 4: the steps either side of `vc` as DEVICE-RESIDENT operations, so that
//   src -> push_delta -> vc -> fvpostf!    (bin/vc.jl:75-82, src/datasets.jl:6-13, src/common.jl:7-63, src/gv.jl:10-15)
// is one upload and one download (round 5 had them as separate host-pointer calls: two more PCIe round trips).
//   vcmi_push_delta / _dev           [src; delta]: delta_t = (x_{t+1} - x_{t-1}) / 2 for 2 <= t <= T-1, the static value at t = 1, T
//   vcmi_push_delta2 / _dev          ... with a third block, delta-delta_t = x_{t-1} - 2 x_t + x_{t+1}, absent neighbours dropped
//   vcmi_variance_scaling / _dev     per row sqrt(sigma2 / var) (x - mean) + mean, Julia's corrected variance, in place allowed
//   vcmi_vc_frames_postf             vc(g::GMMMap, fm) with fvpostf! applied to the converted rows before the download
//   vc_traj_pre_device / vc_traj_post_device   the two ends of vc(c::TrajectoryConverter, fm) around the chunk conversions
//                                    (vc_traj_device in traj_vc.cpp: vcmi_vc_traj_postf, vcmi_vc_traj_static, vcmi_vc_trajgv, *_dev)
// One kernel, vs_scale_kernel, holds fvpostf!'s scale: variance_scaling_device runs it in place or into another matrix,
// vc_traj_post_device into rows 2..D+1 of vc's result.  The host-pointer entries stage whole matrices in the per-thread
// VcScratch (postf.hpp), freed on return above kVcScratchKeepBytes.  Everything is HBM-bound streaming: a frame is D contiguous
// doubles, lanes run along the features of consecutive frames (coalesced), every reduction has a fixed order.
#include "postf.hpp"
#include "gmmmap_handle.hpp"
#include "hostpipe.hpp"

namespace vcmi {

// the delta-delta value of a frame, one expression for the kernel and the host routine: neighbours that exist only (lo: t-1,
// hi: t+1), left to right, no contraction -- the two agree bit for bit
__host__ __device__ static inline double push_delta2_value(bool lo, bool hi, double xm, double x, double xp) {
#pragma clang fp contract(off)
  double a = -2.0 * x;
  if (lo) a = xm + a;
  if (hi) a = a + xp;
  return a;
}

// ---- push_delta, src/datasets.jl:6-13 ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
push_delta_kernel(const double *__restrict__ src, int64_t lds, int D, int64_t T, double *__restrict__ out, int64_t ldo) {
  const int64_t n = (int64_t)D * T;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t t = e / D;
    const int d = (int)(e - t * D);
    const double x = src[t * lds + d];
    out[t * ldo + d] = x;                                          // repmat(src, 2): the static rows, src/datasets.jl:8
    // t = 2:T-1 (1-based): -0.5 x_{t-1} + 0.5 x_{t+1}, src/datasets.jl:9-11; the first and the last frame keep the copy
    out[t * ldo + D + d] = (t >= 1 && t + 1 < T) ? -0.5 * src[(t - 1) * lds + d] + 0.5 * src[(t + 1) * lds + d] : x;
  }
}

int push_delta_device(const double *dsrc, int64_t lds, int D, int64_t T, double *dout, int64_t ldo, hipStream_t st) {
  if (T == 0) return VCMI_OK;
  const int64_t n = (int64_t)D * T;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(push_delta_kernel, dim3(grid), dim3(256), 0, st, dsrc, lds, D, T, dout, ldo);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// ---- push_delta with a delta-delta block: out (3D,T) = [src; delta; delta-delta].  Rows 0 .. 2D-1 are push_delta_kernel's, by the
// same expressions; rows 2D .. 3D-1 are x_{t-1} - 2 x_t + x_{t+1} with a neighbour outside the matrix DROPPED (the convention of
// the trajectory solver's W, traj_penta_step.hpp: a_1 = -2 x_1 + x_2, a_T = x_{T-1} - 2 x_T, T = 1: -2 x_1), summed left to right.
__global__ void __launch_bounds__(256)
push_delta2_kernel(const double *__restrict__ src, int64_t lds, int D, int64_t T, double *__restrict__ out, int64_t ldo) {
#pragma clang fp contract(off)
  const int64_t n = (int64_t)D * T;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t t = e / D;
    const int d = (int)(e - t * D);
    const double x = src[t * lds + d];
    const bool lo = t >= 1, hi = t + 1 < T;
    const double xm = lo ? src[(t - 1) * lds + d] : 0.0, xp = hi ? src[(t + 1) * lds + d] : 0.0;
    out[t * ldo + d] = x;
    out[t * ldo + D + d] = (lo && hi) ? -0.5 * xm + 0.5 * xp : x;
    out[t * ldo + 2 * D + d] = push_delta2_value(lo, hi, xm, x, xp);
  }
}

int push_delta2_device(const double *dsrc, int64_t lds, int D, int64_t T, double *dout, int64_t ldo, hipStream_t st) {
  if (T == 0) return VCMI_OK;
  const int64_t n = (int64_t)D * T;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(push_delta2_kernel, dim3(grid), dim3(256), 0, st, dsrc, lds, D, T, dout, ldo);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// ---- fvpostf!(vs::VarianceScaling, src), src/gv.jl:10-15: three streaming passes (sums, centred squares, scale) over frame
// chunks, every reduction in a fixed order.
//   vs_partial_kernel: part[chunk][d] = sum over the chunk's frames of x (MODE 0) or (x - mean[d])^2 (MODE 1)
//   vs_final_kernel:   stat[d] = sum_chunk part[chunk][d] / denom
static constexpr int kVsChunk = 2048;   // frames per workgroup
template <int MODE>
__global__ void __launch_bounds__(256)
vs_partial_kernel(const double *__restrict__ src, int64_t lds, int D, int64_t T, const double *__restrict__ mean, double *__restrict__ part) {
  extern __shared__ double vred[];       // [NG][D]
  const int tid = threadIdx.x, NG = 256 / D, d = tid % D, g = tid / D;
  const int64_t f0 = (int64_t)blockIdx.x * kVsChunk, f1 = (f0 + kVsChunk < T) ? f0 + kVsChunk : T;
  double s = 0.0;
  if (g < NG) {
    const double m = MODE ? mean[d] : 0.0;
    for (int64_t t = f0 + g; t < f1; t += NG) {
      const double e = src[t * lds + d] - m;
      s = MODE ? fma(e, e, s) : s + e;
    }
    vred[g * D + d] = s;
  }
  __syncthreads();
  if (tid < D) {
    double a = 0.0;
    for (int k = 0; k < NG; ++k) a += vred[k * D + tid];
    part[(size_t)blockIdx.x * D + tid] = a;
  }
}

__global__ void __launch_bounds__(256)
vs_final_kernel(const double *__restrict__ part, int nchunks, int D, double denom, double *__restrict__ stat) {
  const int d = threadIdx.x;
  if (d >= D) return;
  double a = 0.0;
  for (int c = 0; c < nchunks; ++c) a += part[(size_t)c * D + d];
  stat[d] = a / denom;
}

// src (D,T) -> out (D,T), each with its leading dimension; FILTER: through fvpostf!'s scale (src/gv.jl:13) with
// stat = [mean | var | sigma2] of variance_scaling_stats_device, else a copy.  (src and out may be the same matrix: every
// element is read and written by the same thread, hence no __restrict__ on the two.)
template <bool FILTER>
__global__ void __launch_bounds__(256)
vs_scale_kernel(const double *src, int64_t lds, int D, int64_t T, const double *__restrict__ stat, double *out, int64_t ldo) {
  const double *mean = stat, *var = stat + kVsStatStride, *sigma2 = stat + 2 * kVsStatStride;
  const int64_t n = (int64_t)D * T;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t t = e / D;
    const int d = (int)(e - t * D);
    const double x = src[t * lds + d];
    out[t * ldo + d] = FILTER ? sqrt(sigma2[d] / var[d]) * (x - mean[d]) + mean[d] : x;
  }
}

struct VsScratch {
  DevBuf<double> part, stat;     // stat: [mean (D) | var (D) | sigma2 (D)]
  StreamOrder order;
};
static VsScratch &vs_scratch() {
  static thread_local VsScratch s;
  return s;
}

int variance_scaling_stats_device(const double *dsrc, int64_t lds, int D, int64_t T, const double *sigma2_host,
                                  const double **dstat, hipStream_t st) {
  static_assert(kVsStatStride >= 256, "one slot per supported feature row");
  if (D < 1 || D > 256 || T < 2)
    return fail(VCMI_ERR_DIM, "variance scaling: D=%d T=%lld unsupported (needs 1 <= D <= 256, T >= 2)", D, (long long)T);
  VsScratch &sc = vs_scratch();
  const int nchunks = (int)((T + kVsChunk - 1) / kVsChunk);
  VCMI_TRY(sc.part.reserve((size_t)nchunks * D));
  VCMI_TRY(sc.stat.reserve((size_t)3 * kVsStatStride));
  VCMI_TRY(sc.order.enter(st));
  double *mean = sc.stat.p, *var = sc.stat.p + kVsStatStride, *sig = sc.stat.p + 2 * kVsStatStride;
  // (D doubles from pageable memory: the runtime stages them before returning, the caller's vector is free at once)
  VCMI_HIP(hipMemcpyAsync(sig, sigma2_host, sizeof(double) * D, hipMemcpyHostToDevice, st));
  const size_t shm = (size_t)(256 / D) * D * sizeof(double);
  hipLaunchKernelGGL(vs_partial_kernel<0>, dim3(nchunks), dim3(256), shm, st, dsrc, lds, D, T, mean, sc.part.p);
  hipLaunchKernelGGL(vs_final_kernel, dim3(1), dim3(256), 0, st, sc.part.p, nchunks, D, (double)T, mean);
  hipLaunchKernelGGL(vs_partial_kernel<1>, dim3(nchunks), dim3(256), shm, st, dsrc, lds, D, T, mean, sc.part.p);
  hipLaunchKernelGGL(vs_final_kernel, dim3(1), dim3(256), 0, st, sc.part.p, nchunks, D, (double)(T - 1), var);   // Julia's var
  VCMI_HIP(hipGetLastError());
  *dstat = sc.stat.p;
  return VCMI_OK;
}

int variance_scaling_stats_leave(hipStream_t st) { return vs_scratch().order.leave(st); }

int variance_scaling_device(const double *dsrc, int64_t lds, int D, int64_t T, const double *sigma2_host, double *dout,
                            int64_t ldo, hipStream_t st) {
  const double *stat = nullptr;
  VCMI_TRY(variance_scaling_stats_device(dsrc, lds, D, T, sigma2_host, &stat, st));
  hipLaunchKernelGGL(vs_scale_kernel<true>, dim3(2048), dim3(256), 0, st, dsrc, lds, D, T, stat, dout, ldo);
  VCMI_HIP(hipGetLastError());
  return variance_scaling_stats_leave(st);
}

// ---- the two ends of vc(c::TrajectoryConverter, fm) around the chunk conversions, bin/vc.jl:75-82 + src/common.jl:31-63 ------
// vc_traj_pre_kernel: fm (rows,T), leading dimension ldf, read once -> x (2D,T) dense, the converter's input, and the power row
// into `out` (skipped when out is NULL: the caller assembles the result in place in fm, the row is already there).
//   STATIC: rows = D+1; x = [fm[2:end,:]; delta], the delta over the WHOLE matrix with push_delta_kernel's arithmetic (the
//           first and the last frame of the matrix -- not of a chunk -- keep the copy), bin/vc.jl:77-78, src/datasets.jl:6-13
//   else:   rows = D2+1, D2 = dim(t) (2D; 3D for a converter with three windows); x = fm[2:end,:] (D2,T)
template <bool STATIC>
__global__ void __launch_bounds__(256)
vc_traj_pre_kernel(const double *__restrict__ fm, int64_t ldf, int D, int D2, int64_t T, double *__restrict__ x, double *__restrict__ out,
                   int64_t ldo) {
  const int R = STATIC ? D : D2;                                     // feature rows read per frame
  const int64_t n = (int64_t)R * T;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t t = e / R;
    const int d = (int)(e - t * R);
    const double *src = fm + 1;                                      // row 2 of fm: the first feature row
    const double v = src[t * ldf + d];
    if (STATIC) {
      x[t * 2 * D + d] = v;
      x[t * 2 * D + D + d] = (t >= 1 && t + 1 < T) ? -0.5 * src[(t - 1) * ldf + d] + 0.5 * src[(t + 1) * ldf + d] : v;
    } else {
      x[e] = v;
    }
    if (d == 0 && out) out[t * ldo] = fm[t * ldf];                   // power row kept, src/common.jl:60
  }
}

int vc_traj_pre_device(const double *dfm, int64_t ldf, int D, int D2, int64_t T, bool is_static, double *dx, double *dout, int64_t ldo,
                       hipStream_t st) {
  if (T == 0) return VCMI_OK;
  const int64_t n = (int64_t)(is_static ? D : D2) * T;
  const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, 8192));
  if (is_static) hipLaunchKernelGGL(vc_traj_pre_kernel<true>, grid, dim3(256), 0, st, dfm, ldf, D, D2, T, dx, dout, ldo);
  else hipLaunchKernelGGL(vc_traj_pre_kernel<false>, grid, dim3(256), 0, st, dfm, ldf, D, D2, T, dx, dout, ldo);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// y (D,T) dense -> rows 2..D+1 of out (leading dimension ldo), through fvpostf!'s scale when dstat is given
int vc_traj_post_device(const double *dy, int D, int64_t T, const double *dstat, double *dout, int64_t ldo, hipStream_t st) {
  if (T == 0) return VCMI_OK;
  const int64_t n = (int64_t)D * T;
  const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, 8192));
  if (dstat) hipLaunchKernelGGL(vs_scale_kernel<true>, grid, dim3(256), 0, st, dy, (int64_t)D, D, T, dstat, dout + 1, ldo);
  else hipLaunchKernelGGL(vs_scale_kernel<false>, grid, dim3(256), 0, st, dy, (int64_t)D, D, T, dstat, dout + 1, ldo);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

VcScratch &vc_scratch() {
  static thread_local VcScratch s;
  return s;
}

}  // namespace vcmi

using namespace vcmi;

extern "C" int vcmi_push_delta_dev(const double *dsrc, int64_t lds, int D, int64_t T, double *dout, int64_t ldo, void *stream) {
  if (D < 1 || T < 0 || lds < D || ldo < 2 * (int64_t)D) return fail(VCMI_ERR_ARG, "vcmi_push_delta_dev: bad argument");
  if (T > 0 && (!dsrc || !dout)) return fail(VCMI_ERR_ARG, "vcmi_push_delta_dev: NULL argument");
  VCMI_TRY(check_device());
  return push_delta_device(dsrc, lds, D, T, dout, ldo, as_stream(stream));
}

// push_delta(src (D,T)) -> out (2D,T) on HOST matrices: host arithmetic -- three streaming passes over memory the caller already
// holds cost less than moving the matrix over PCIe and back (and the helper works without a device); the device-resident
// form above is the one the vc pipeline uses
// (ldo: the rows of out, 2D here and 3D under vcmi_push_delta2)
static void push_delta_host(const double *src, int D, int64_t T, double *out, size_t ldo) {
  for (int64_t t = 0; t < T; ++t)
    for (int d = 0; d < D; ++d) {   // repmat(src, 2), src/datasets.jl:8
      out[d + ldo * t] = src[d + (size_t)D * t];
      out[D + d + ldo * t] = src[d + (size_t)D * t];
    }
  for (int64_t t = 1; t + 1 < T; ++t)   // t = 2:T-1, src/datasets.jl:9-11
    for (int d = 0; d < D; ++d)
      out[D + d + ldo * t] = -0.5 * src[d + (size_t)D * (t - 1)] + 0.5 * src[d + (size_t)D * (t + 1)];
}

extern "C" int vcmi_push_delta(const double *src, int D, int64_t T, double *out) {
  if (!src || !out || D < 1 || T < 0) return fail(VCMI_ERR_ARG, "vcmi_push_delta: bad argument");
  push_delta_host(src, D, T, out, (size_t)2 * D);
  return VCMI_OK;
}

// push_delta(src (D,T), order = 2) -> out (3D,T): rows 0 .. 2D-1 as vcmi_push_delta makes them, rows 2D .. 3D-1 the delta-delta
// rows of push_delta2_kernel.  Host arithmetic, like vcmi_push_delta.
extern "C" int vcmi_push_delta2(const double *src, int D, int64_t T, double *out) {
  if (!src || !out || D < 1 || T < 0) return fail(VCMI_ERR_ARG, "vcmi_push_delta2: bad argument");
  push_delta_host(src, D, T, out, (size_t)3 * D);
  for (int64_t t = 0; t < T; ++t)
    for (int d = 0; d < D; ++d) {
      const bool lo = t >= 1, hi = t + 1 < T;
      out[2 * D + d + (size_t)3 * D * t] = push_delta2_value(lo, hi, lo ? src[d + (size_t)D * (t - 1)] : 0.0, src[d + (size_t)D * t],
                                                             hi ? src[d + (size_t)D * (t + 1)] : 0.0);
    }
  return VCMI_OK;
}

extern "C" int vcmi_push_delta2_dev(const double *dsrc, int64_t lds, int D, int64_t T, double *dout, int64_t ldo, void *stream) {
  if (D < 1 || T < 0 || lds < D || ldo < 3 * (int64_t)D) return fail(VCMI_ERR_ARG, "vcmi_push_delta2_dev: bad argument");
  if (T > 0 && (!dsrc || !dout)) return fail(VCMI_ERR_ARG, "vcmi_push_delta2_dev: NULL argument");
  VCMI_TRY(check_device());
  return push_delta2_device(dsrc, lds, D, T, dout, ldo, as_stream(stream));
}

extern "C" int vcmi_variance_scaling_dev(const double *dsrc, int64_t lds, int D, int64_t T, const double *sigma2, double *dout,
                                         int64_t ldo, void *stream) {
  if (!dsrc || !sigma2 || !dout) return fail(VCMI_ERR_ARG, "vcmi_variance_scaling_dev: NULL argument");
  if (lds < D || ldo < D) return fail(VCMI_ERR_ARG, "vcmi_variance_scaling_dev: leading dimension below D");
  VCMI_TRY(check_device());
  return variance_scaling_device(dsrc, lds, D, T, sigma2, dout, ldo, as_stream(stream));
}

// fvpostf(vs::VarianceScaling, src) -- src/gv.jl:10-21.  src, out (D,T) host matrices (may alias), sigma2 (D).
extern "C" int vcmi_variance_scaling(const double *src, int D, int64_t T, const double *sigma2, double *out) {
  if (!src || !sigma2 || !out) return fail(VCMI_ERR_ARG, "vcmi_variance_scaling: NULL argument");
  if (D < 1 || D > 256 || T < 2)
    return fail(VCMI_ERR_DIM, "vcmi_variance_scaling: D=%d T=%lld unsupported (needs 1 <= D <= 256, T >= 2)", D, (long long)T);
  VCMI_TRY(check_device());
  VcScratch &sc = vc_scratch();
  VcScratch::Release release{sc};
  VCMI_TRY(sc.stage.reserve((size_t)D * T));
  VCMI_TRY(staged_upload(sc.stage.p, src, sizeof(double) * D * T, nullptr));
  VCMI_TRY(variance_scaling_device(sc.stage.p, D, D, T, sigma2, sc.stage.p, D, nullptr));
  return staged_download(out, sc.stage.p, sizeof(double) * D * T, nullptr);
}

// vc(g::GMMMap, fm) followed by fvpostf!(VarianceScaling(sigma2), converted[2:end, :]) -- src/common.jl:7-26, src/gv.jl:10-15:
// fm, out (D+1,T) host matrices, row 1 (power) passed through.  The post-filter needs the mean and variance of every converted
// row over the WHOLE matrix, so the matrix stays on the device between the two steps: one upload, one download.  (Runs on the
// calling thread's device: a device group does not shard it -- the statistics would need a collective for a 0.1 ms step.)
extern "C" int vcmi_vc_frames_postf(vcmi_gmmmap *g, const double *fm, int64_t T, const double *sigma2, double *out) {
  if (!sigma2) return vcmi_vc_frames(g, fm, T, out);
  if (!g) return fail(VCMI_ERR_ARG, "vcmi_vc_frames_postf: NULL handle");
  if (T < 0 || (T > 0 && (!fm || !out))) return fail(VCMI_ERR_ARG, "vcmi_vc_frames_postf: bad argument");
  if (T == 0) return VCMI_OK;
  if (T < 2) return fail(VCMI_ERR_DIM, "vcmi_vc_frames_postf: the variance of a one-frame matrix is undefined");
  VCMI_TRY(check_device());
  const int64_t ld = g->D + 1;
  const size_t bytes = sizeof(double) * (size_t)ld * T;
  VcScratch &sc = vc_scratch();
  VcScratch::Release release{sc};
  VCMI_TRY(sc.stage.reserve((size_t)2 * ld * T));                    // fm, and the result behind it
  double *din = sc.stage.p, *dout = sc.stage.p + (size_t)ld * T;
  VCMI_TRY(staged_upload(din, fm, bytes, nullptr));
  // the copy keeps row 1 (src/common.jl:23); the kernel then overwrites rows 2..D+1, as in vcmi_vc_frames
  VCMI_HIP(hipMemcpyAsync(dout, din, bytes, hipMemcpyDeviceToDevice, nullptr));
  VCMI_TRY(gmmmap_convert_device(g, din + 1, ld, T, dout + 1, ld, nullptr));
  VCMI_TRY(variance_scaling_device(dout + 1, ld, g->D, T, sigma2, dout + 1, ld, nullptr));
  return staged_download(out, dout, bytes, nullptr);
}
