// traj_gv_band.hip -- the global-variance ascent (traj_gv.hip's header; reference src/trajectory_gmmmap.jl:139-189) over DIAGONAL
// conditional precisions: traj_gvd_kernel for a converter with two windows (behind traj_diag.hip's solve), traj_gvp_kernel for one
// with three (static + delta + delta-delta, vcmi_traj_create_bdiag_windows; behind traj_penta.hip's), and their one launch.  Both
// kernels are the frame of traj_gv_band.hpp around a stencil.  The handle and the checks of a call stay in traj_gv.hip
// (vcmi_trajgv_create_diag / _bdiag, trajgv_args); the launch rule is host arithmetic of its own (traj_band_plan.hpp).
#include "traj_gv_band.hpp"

namespace vcmi {

template <int NRES>
__global__ void __launch_bounds__(kGvdThreads)
traj_gvd_kernel(const TrajUtt *__restrict__ utts, int n, int D, int64_t lds_arr, const double *__restrict__ q,
                const int64_t *__restrict__ mhat_all, const double *__restrict__ g_all, double *__restrict__ ws_gv, int64_t nframes,
                TrajGV gv) {
  traj_gv_band<GvdStencil<NRES>, NRES>(blockDim.x, utts, n, D, lds_arr, q, mhat_all, g_all, ws_gv, nframes, gv);
}

template <int NRES>
__global__ void __launch_bounds__(kGvdThreads)
traj_gvp_kernel(const TrajUtt *__restrict__ utts, int n, int D, int64_t lds_arr, const double *__restrict__ q,
                const int64_t *__restrict__ mhat_all, const double *__restrict__ g_all, double *__restrict__ ws_gv, int64_t nframes,
                TrajGV gv) {
  traj_gv_band<GvpStencil<NRES>, NRES>(blockDim.x, utts, n, D, lds_arr, q, mhat_all, g_all, ws_gv, nframes, gv);
}

// [windows - 2][arrays resident in LDS]; one array alone is never resident (band_resident)
typedef void (*BandGvKernel)(const TrajUtt *, int, int, int64_t, const double *, const int64_t *, const double *, double *, int64_t, TrajGV);
static const BandGvKernel kBandGvKernels[2][kGvpArrays + 1] = {
    {traj_gvd_kernel<0>, nullptr, traj_gvd_kernel<2>, traj_gvd_kernel<3>, traj_gvd_kernel<4>, traj_gvd_kernel<5>, nullptr},
    {traj_gvp_kernel<0>, nullptr, traj_gvp_kernel<2>, traj_gvp_kernel<3>, traj_gvp_kernel<4>, traj_gvp_kernel<5>, traj_gvp_kernel<6>}};

int traj_band_gv_launch(vcmi_traj *t, const TrajSolvePlan &p, const TrajGV &gv, hipStream_t st) {
  const int D = t->D, W = t->windows;
  const char *who = W == 3 ? "BlockDiagTrajectoryGVGMMMap" : "DiagTrajectoryGVGMMMap";
  if (D > kGvdThreads) return fail(VCMI_ERR_ARG, "%s: static dimension %d beyond %d", who, D, kGvdThreads);
  // the kernel writes its arrays 1 .. (nframes,D each) into the workspace: the plan of a call with GV reserves them (traj_solve_plan)
  const int64_t need = band_ws_doubles(W, p.nframes, D, true);
  if (p.ws_stride < need)
    return fail(VCMI_ERR_ARG, "%s: workspace of %lld doubles below %lld", who, (long long)p.ws_stride, (long long)need);
  const int arrays = band_gv_arrays(W);
  const BandGvKernel kern = kBandGvKernels[W - 2][band_resident(arrays, D, p.Tmax)];
  const size_t shmem = band_lds_bytes(arrays, D, p.Tmax);
  VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(kern, dim3(p.grid), dim3(kGvdThreads), shmem, st, p.du, p.n, D, (int64_t)p.Tmax * D, t->dg_q.p, t->mhat.p, t->gbuf.p,
                     t->ws.p + band_gv_ws_offset(W, 1, p.nframes, D), p.nframes, gv);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

}  // namespace vcmi
