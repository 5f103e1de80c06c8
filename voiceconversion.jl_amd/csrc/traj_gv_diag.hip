// traj_gv_diag.hip -- the global-variance ascent (traj_gv.hip's header; reference src/trajectory_gmmmap.jl:139-189) over DIAGONAL
// conditional precisions: traj_gvd_kernel and its launch.  The handle and the checks of a call stay in traj_gv.hip
// (vcmi_trajgv_create_diag, trajgv_args); the launch rule is host arithmetic of its own (traj_gvd_plan.hpp).
//
// With D^-1 = diag(q), q[mhat_t] = [p_s(t) ; p_d(t)], the likelihood gradient of traj_gv.hip loses the product with Q_m: per
// static dimension d (traj_diag.hip's header, the matrix its solver factorises)
//   (P y)_t = c0_t y_t + c2_t y_{t-2} + c2_{t+2} y_{t+2}      c0_t = p_s(t) + p_d(t-1)/4 + p_d(t+1)/4,   c2_t = -p_d(t-1)/4
//   r_t     = g_s(t) + g_d(t-1)/2 - g_d(t+1)/2
// with W's boundaries: a p_d of a frame outside the utterance is absent everywhere; a y_{t-2} / y_{t+2} outside the utterance is
// absent (c2_t is stored as 0 for t < 2, c2_{t+2} is not read for t + 2 >= T) while the p_d(t-1)/4 y_t that goes with the
// existing frame t-1 stays in c0.  The epoch
//   y <- y + alpha ( omega (r - P y) + coef (.) (y - mean) ),   coef = -2/T pv' (var_1(y) - mu_v),   omega = 1/(2T)
// is a JACOBI step: y_{t+-2} are the previous epoch's, so y has two buffers that swap per epoch.
#include "traj_internal.hpp"
#include "traj_gv_moments.hpp"
#include "traj_gvd_plan.hpp"
#include "traj_gv_sel.hpp"      // GvdPtr / gvd_sel: an array in LDS or in global memory, per instantiation

namespace vcmi {

static constexpr int kGvdBatch = 4;   // independent frames a thread has in flight in the epoch: 7 loads each

// ------------------------------------------------------------------------------------------------
// One workgroup per utterance (persistent loop over the call's utterances) runs all epochs; pv' (var - mu_v) couples all static
// dimensions once per epoch, so an utterance is not split.  Thread = (dimension d = tid % D, phase = tid / D) walks the frames
// phase, phase + NG, ... (NG = 512 / D): d is fastest across the lanes, a wave reads and writes whole rows of (T,D) arrays.
//   prologue, once per utterance: the two-pass moments of the solved trajectory, then ONE pass that rescales y by eq. (58) and
//     writes c0, c2 and r -- the dependent gathers q[mhat_{t-1}], q[mhat_t], q[mhat_{t+1}] happen here and nowhere else;
//   epoch: the update above from `src` into `dst`, kGvdBatch frames per thread in flight on clamped addresses; the pass that
//     writes the new y accumulates its moments as shifted sums about the previous mean, reduced over the phases in a fixed
//     order (no atomics); then mean, var and coef for the next epoch.  Three barriers per epoch.
// NRES of the five arrays (y, second y, c2, c0, r -- traj_gvd_plan.hpp) are in LDS across the epochs, the others in the workspace
// (the first y then is the utterance's Y itself).  The arithmetic does not depend on NRES: an utterance's bits are the same in
// every batch.  After the last epoch the result is in Y: copied out of LDS, or, streamed, by starting in the buffer whose parity
// ends there.  Contraction is off: what is fused is written as fma.
// ------------------------------------------------------------------------------------------------
template <int NRES>
__global__ void __launch_bounds__(kGvdThreads)
traj_gvd_kernel(const TrajUtt *__restrict__ utts, int n, int D, int64_t lds_arr, const double *__restrict__ q,
                const int64_t *__restrict__ mhat_all, const double *__restrict__ g_all, double *__restrict__ ws_gv, int64_t nframes,
                TrajGV gv) {
#pragma clang fp contract(off)
  static_assert(NRES == 0 || (NRES >= 2 && NRES <= kGvdArrays), "arrays resident in LDS");
  extern __shared__ double gsm[];
  const int D2 = 2 * D, nthr = blockDim.x;
  double *red = gsm;                       // [2][nthr]
  double *mean = red + 2 * nthr;           // [D]
  double *var = mean + D;                  // [D]
  double *coef = var + D;                  // [D]
  double *arr = coef + D;                  // [NRES][lds_arr]
  const int tid = threadIdx.x;
  const int NG = nthr / D, d = tid % D, ph = tid / D;
  const bool act = ph < NG;
  typedef typename GvdPtr<(NRES >= 2)>::type YP;

  for (int u = blockIdx.x; u < n; u += gridDim.x) {
    const TrajUtt U = utts[u];
    const int T = U.T;
    if (T < 2) continue;                   // var() of one frame is undefined; the host rejects such calls
    const int64_t *mh = mhat_all + U.frame0;
    const double *g = g_all + U.frame0 * D2;
    gdouble *Yg = (gdouble *)U.Y;
    gdouble *wsu = (gdouble *)ws_gv + U.frame0 * D;
    // streamed, the ascent starts in the buffer from which `epochs` swaps end in Y
    YP src = gvd_sel<(NRES >= 2)>(arr, (gv.epochs & 1) ? wsu : Yg);
    YP dst = gvd_sel<(NRES >= 2)>(arr + lds_arr, (gv.epochs & 1) ? Yg : wsu);
    const auto C2 = gvd_sel<(NRES >= 3)>(arr + 2 * lds_arr, wsu + nframes * D);
    const auto C0 = gvd_sel<(NRES >= 4)>(arr + 3 * lds_arr, wsu + 2 * nframes * D);
    const auto R = gvd_sel<(NRES >= 5)>(arr + 4 * lds_arr, wsu + 3 * nframes * D);
    const double omega = 1.0 / (2.0 * (double)T);

    gv_moments(Yg, D, T, nthr, red, mean, var);
    // moments of the y just written from the shifted sums of the pass (traj_gv_kernel), then the gvgrad coefficients of the
    // next epoch, src/trajectory_gmmmap.jl:171-189: -2/T (pv' (var(y) - mu^v))
    auto finish = [&](double s1, double s2) {
      if (act) {
        red[ph * D + d] = s1;
        red[nthr + ph * D + d] = s2;
      }
      __syncthreads();
      if (tid < D) {
        double a1 = 0.0, a2 = 0.0;
        for (int k = 0; k < NG; ++k) {
          a1 += red[k * D + tid];
          a2 += red[nthr + k * D + tid];
        }
        mean[tid] += a1 / (double)T;
        var[tid] = (a2 - a1 * a1 / (double)T) / (double)(T - 1);       // Julia's var: corrected
      }
      __syncthreads();
      if (tid < D) {
        double s = 0.0;
        for (int j = 0; j < D; ++j) s = fma(gv.pv[j + (size_t)D * tid], var[j] - gv.muv[j], s);
        coef[tid] = -2.0 / (double)T * s;
      }
      __syncthreads();
    };

    // eq. (58): y <- sqrt(mu^v / var(y)) (y - mean) + mean, src/trajectory_gmmmap.jl:152; c0, c2 and r
    {
      double s1 = 0.0, s2 = 0.0;
      if (act) {
        const double mu = mean[d], sc = sqrt(gv.muv[d] / var[d]);
#pragma unroll 4
        for (int t = ph; t < T; t += NG) {
          const size_t e = (size_t)t * D + d;
          const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
          const int m0 = (int)mh[t] - 1, mm = (int)mh[tm] - 1, mp = (int)mh[tp] - 1;
          const double ps = q[(size_t)m0 * D2 + d], pdm = q[(size_t)mm * D2 + D + d], pdp = q[(size_t)mp * D2 + D + d];
          const double yo = Yg[e], g0 = g[(size_t)t * D2 + d], g1 = g[(size_t)tm * D2 + D + d], g2 = g[(size_t)tp * D2 + D + d];
          const double yn = sc * (yo - mu) + mu;
          src[e] = yn;
          R[e] = (g0 + (t >= 1 ? 0.5 : 0.0) * g1) - (t + 1 < T ? 0.5 : 0.0) * g2;
          C0[e] = (ps + (t >= 1 ? 0.25 : 0.0) * pdm) + (t + 1 < T ? 0.25 : 0.0) * pdp;
          C2[e] = t >= 2 ? -0.25 * pdm : 0.0;
          const double dv = yn - mu;
          s1 += dv;
          s2 = fma(dv, dv, s2);
        }
      }
      finish(s1, s2);
    }

    for (int ep = 0; ep < gv.epochs; ++ep) {
      double s1 = 0.0, s2 = 0.0;
      if (act) {
        const double mu = mean[d], cf = coef[d];
        for (int t0 = ph; t0 < T; t0 += kGvdBatch * NG) {
          double yc[kGvdBatch], ym[kGvdBatch], yp[kGvdBatch], rr[kGvdBatch], a0[kGvdBatch], am[kGvdBatch], ap[kGvdBatch];
          // every load unconditional, on an address clamped into the utterance: c2 of a frame below 2 is zero, c2_{t+2} of a
          // frame past the end gets weight zero below
#pragma unroll
          for (int k = 0; k < kGvdBatch; ++k) {
            const int t = t0 + k * NG, tc = t < T ? t : T - 1;
            const int tm = tc >= 2 ? tc - 2 : tc, tp = tc + 2 < T ? tc + 2 : tc;
            const size_t ec = (size_t)tc * D + d, em = (size_t)tm * D + d, ep2 = (size_t)tp * D + d;
            yc[k] = src[ec];
            ym[k] = src[em];
            yp[k] = src[ep2];
            rr[k] = R[ec];
            a0[k] = C0[ec];
            am[k] = C2[ec];
            ap[k] = C2[ep2];
          }
#pragma unroll
          for (int k = 0; k < kGvdBatch; ++k) {
            const int t = t0 + k * NG;
            if (t < T) {
              const double wp = t + 2 < T ? ap[k] : 0.0;
              const double py = fma(wp, yp[k], fma(am[k], ym[k], a0[k] * yc[k]));
              // y <- y + alpha ( omega (r - P y) + coef (y - mean) ), eq. (52), src/trajectory_gmmmap.jl:163-166
              const double dy = fma(cf, yc[k] - mu, omega * (rr[k] - py));
              const double yn = fma(gv.alpha, dy, yc[k]);
              dst[(size_t)t * D + d] = yn;
              const double dv = yn - mu;
              s1 += dv;
              s2 = fma(dv, dv, s2);
            }
          }
        }
      }
      finish(s1, s2);       // (its first barrier is also the one between this epoch's reads of src and the next one's writes)
      const YP sw = src;
      src = dst;
      dst = sw;
    }
    if constexpr (NRES >= 2) {
      for (size_t e = tid; e < (size_t)T * D; e += nthr) Yg[e] = src[e];
      __syncthreads();                     // the next utterance writes the same LDS
    }
  }
}

int traj_gvd_launch(vcmi_traj *t, const TrajSolvePlan &p, const TrajGV &gv, hipStream_t st) {
  const int D = t->D;
  if (D > kGvdThreads) return fail(VCMI_ERR_ARG, "DiagTrajectoryGVGMMMap: static dimension %d beyond %d", D, kGvdThreads);
  // the kernel writes four (nframes,D) arrays behind the solver's: the plan of a call with GV reserves them (traj_solve_plan)
  const int64_t need = gvd_ws_doubles(p.nframes, D, true);
  if (p.ws_stride < need)
    return fail(VCMI_ERR_ARG, "DiagTrajectoryGVGMMMap: workspace of %lld doubles below %lld", (long long)p.ws_stride, (long long)need);
  const int nres = gvd_resident(D, p.Tmax);
  const size_t shmem = gvd_lds_bytes(D, p.Tmax);
  auto kern = nres == 5 ? traj_gvd_kernel<5> : nres == 4 ? traj_gvd_kernel<4> : nres == 3 ? traj_gvd_kernel<3>
            : nres == 2 ? traj_gvd_kernel<2> : traj_gvd_kernel<0>;
  VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(kern, dim3(p.grid), dim3(kGvdThreads), shmem, st, p.du, p.n, D, (int64_t)p.Tmax * D, t->dg_q.p, t->mhat.p, t->gbuf.p,
                     t->ws.p + p.nframes * D, p.nframes, gv);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

}  // namespace vcmi
