// traj_gv_penta.hip -- the global-variance ascent (traj_gv.hip's header; reference src/trajectory_gmmmap.jl:139-189) over a
// converter with THREE windows (static + delta + delta-delta, vcmi_traj_create_bdiag_windows): traj_gvp_kernel and its launch.
// The handle and the checks of a call stay in traj_gv.hip (vcmi_trajgv_create_bdiag, trajgv_args); the per-element arithmetic is
// traj_gvp_step.hpp (shared with the host check), the launch rule host arithmetic of its own (traj_gvp_plan.hpp).
//
// With D^-1 = diag(q), q[mhat_t] = [p_s(t) ; p_d(t) ; p_a(t)], the likelihood gradient per static dimension is omega (r - P y)
// with the symmetric pentadiagonal P and the r that traj_penta_solve_kernel solves (traj_penta_step.hpp), read by column:
//   (P y)_t = c0_t y_t + c1_t y_{t-1} + c1_{t+1} y_{t+1} + c2_t y_{t-2} + c2_{t+2} y_{t+2}
// (traj_gvp_step.hpp states c0, c1, c2, r and the boundaries).  The epoch
//   y <- y + alpha ( omega (r - P y) + coef (.) (y - mean) ),   coef = -2/T pv' (var_1(y) - mu_v),   omega = 1/(2T)
// is a JACOBI step: with y_{t+-1} in the stencil an in-place update is wrong at every frame, so y has two buffers that swap per
// epoch.
#include "traj_internal.hpp"
#include "traj_gv_moments.hpp"
#include "traj_gv_sel.hpp"
#include "traj_gvp_plan.hpp"
#include "traj_gvp_step.hpp"

namespace vcmi {

static constexpr int kGvpBatch = 4;   // independent frames a thread has in flight in the epoch: 11 loads each

// ------------------------------------------------------------------------------------------------
// The shape of traj_gvd_kernel (traj_gv_diag.hip).  One workgroup per utterance (persistent loop over the call's utterances) runs
// all epochs; thread = (dimension d = tid % D, phase = tid / D) walks the frames phase, phase + NG, ... (NG = 512 / D): d is
// fastest across the lanes, a wave reads and writes whole rows of (T,D) arrays.
//   prologue, once per utterance: the two-pass moments of the solved trajectory, then ONE pass that rescales y by eq. (58) and
//     writes c0, c1, c2 and r -- the dependent gathers q[mhat_{t-1}], q[mhat_t], q[mhat_{t+1}] happen here and nowhere else;
//   epoch: gvp_epoch_step from `src` into `dst`, kGvpBatch frames per thread in flight on clamped addresses (five y, c0, two c1,
//     two c2, r per element); the pass that writes the new y accumulates its moments as shifted sums about the previous mean,
//     reduced over the phases in a fixed order (no atomics); then mean, var and coef for the next epoch.  Three barriers per epoch.
// NRES of the six arrays (y, second y, c1, c2, c0, r -- traj_gvp_plan.hpp) are in LDS across the epochs, the others in the
// workspace (the first y then is the utterance's Y itself; the second y lies on the solver's l1, c1 on its l2: both are dead
// once the solve has run).  The arithmetic does not depend on NRES: an utterance's bits are the same in every batch.  After the
// last epoch the result is in Y: copied out of LDS, or, streamed, by starting in the buffer whose parity ends there.
// ------------------------------------------------------------------------------------------------
template <int NRES>
__global__ void __launch_bounds__(kGvdThreads)
traj_gvp_kernel(const TrajUtt *__restrict__ utts, int n, int D, int64_t lds_arr, const double *__restrict__ q,
                const int64_t *__restrict__ mhat_all, const double *__restrict__ g_all, double *__restrict__ ws_gv, int64_t nframes,
                TrajGV gv) {
#pragma clang fp contract(off)
  static_assert(NRES == 0 || (NRES >= 2 && NRES <= kGvpArrays), "arrays resident in LDS");
  extern __shared__ double gsm[];
  const int D3 = 3 * D, nthr = blockDim.x;
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
    const double *g = g_all + U.frame0 * D3;
    gdouble *Yg = (gdouble *)U.Y;
    gdouble *wsu = (gdouble *)ws_gv + U.frame0 * D;
    // streamed, the ascent starts in the buffer from which `epochs` swaps end in Y
    YP src = gvd_sel<(NRES >= 2)>(arr, (gv.epochs & 1) ? wsu : Yg);
    YP dst = gvd_sel<(NRES >= 2)>(arr + lds_arr, (gv.epochs & 1) ? Yg : wsu);
    const auto C1 = gvd_sel<(NRES >= 3)>(arr + 2 * lds_arr, wsu + nframes * D);
    const auto C2 = gvd_sel<(NRES >= 4)>(arr + 3 * lds_arr, wsu + 2 * nframes * D);
    const auto C0 = gvd_sel<(NRES >= 5)>(arr + 4 * lds_arr, wsu + 3 * nframes * D);
    const auto R = gvd_sel<(NRES >= 6)>(arr + 5 * lds_arr, wsu + 4 * nframes * D);
    const double omega = 1.0 / (2.0 * (double)T);

    gv_moments(Yg, D, T, nthr, red, mean, var);
    // moments of the y just written from the shifted sums of the pass (traj_gvd_kernel), then the gvgrad coefficients of the
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

    // eq. (58): y <- sqrt(mu^v / var(y)) (y - mean) + mean, src/trajectory_gmmmap.jl:152; c0, c1, c2 and r
    {
      double s1 = 0.0, s2 = 0.0;
      if (act) {
        const double mu = mean[d], sc = sqrt(gv.muv[d] / var[d]);
#pragma unroll 2
        for (int t = ph; t < T; t += NG) {
          const size_t e = (size_t)t * D + d;
          const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
          const double *q0 = q + (size_t)((int)mh[t] - 1) * D3 + d, *qm = q + (size_t)((int)mh[tm] - 1) * D3 + d,
                       *qp = q + (size_t)((int)mh[tp] - 1) * D3 + d;
          const double *g0 = g + (size_t)t * D3 + d, *gm = g + (size_t)tm * D3 + d, *gp = g + (size_t)tp * D3 + d;
          const PentaRow cur{q0[0], q0[D], q0[2 * D], g0[0], g0[D], g0[2 * D]};
          const PentaRow prv{0.0, qm[D], qm[2 * D], 0.0, gm[D], gm[2 * D]};     // (the static parts of a neighbour are not read)
          const PentaRow nxt{0.0, qp[D], qp[2 * D], 0.0, gp[D], gp[2 * D]};
          const double yo = Yg[e];
          const GvpCoef c = gvp_coefficients(prv, cur, nxt, t, T);
          const double yn = sc * (yo - mu) + mu;
          src[e] = yn;
          C0[e] = c.c0;
          C1[e] = c.c1;
          C2[e] = c.c2;
          R[e] = c.r;
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
        for (int t0 = ph; t0 < T; t0 += kGvpBatch * NG) {
          double y0[kGvpBatch], ym1[kGvpBatch], yp1[kGvpBatch], ym2[kGvpBatch], yp2[kGvpBatch], rr[kGvpBatch], a0[kGvpBatch],
              a1[kGvpBatch], a1n[kGvpBatch], a2[kGvpBatch], a2n[kGvpBatch];
          // every load unconditional, on an address clamped into the utterance (T >= 2): c1 of frame 0 and c2 of a frame below 2
          // are stored as zero, what is loaded for a frame past the end gets weight zero in gvp_epoch_step
#pragma unroll
          for (int k = 0; k < kGvpBatch; ++k) {
            const int t = t0 + k * NG, tc = t < T ? t : T - 1;
            const int t1m = tc >= 1 ? tc - 1 : tc, t1p = tc + 1 < T ? tc + 1 : tc;
            const int t2m = tc >= 2 ? tc - 2 : tc, t2p = tc + 2 < T ? tc + 2 : tc;
            const size_t ec = (size_t)tc * D + d, e1m = (size_t)t1m * D + d, e1p = (size_t)t1p * D + d, e2m = (size_t)t2m * D + d,
                         e2p = (size_t)t2p * D + d;
            y0[k] = src[ec];
            ym1[k] = src[e1m];
            yp1[k] = src[e1p];
            ym2[k] = src[e2m];
            yp2[k] = src[e2p];
            rr[k] = R[ec];
            a0[k] = C0[ec];
            a1[k] = C1[ec];
            a1n[k] = C1[e1p];
            a2[k] = C2[ec];
            a2n[k] = C2[e2p];
          }
#pragma unroll
          for (int k = 0; k < kGvpBatch; ++k) {
            const int t = t0 + k * NG;
            if (t < T) {
              const double yn = gvp_epoch_step(y0[k], ym1[k], yp1[k], ym2[k], yp2[k], a0[k], a1[k], a1n[k], a2[k], a2n[k], rr[k], t, T,
                                               omega, cf, mu, gv.alpha);
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

int traj_gvp_launch(vcmi_traj *t, const TrajSolvePlan &p, const TrajGV &gv, hipStream_t st) {
  const int D = t->D;
  if (D > kGvdThreads) return fail(VCMI_ERR_ARG, "BlockDiagTrajectoryGVGMMMap: static dimension %d beyond %d", D, kGvdThreads);
  // the kernel writes five (nframes,D) arrays from the start of the workspace: the plan of a three-window call with GV
  // reserves them (traj_solve_plan)
  const int64_t need = gvp_ws_doubles(p.nframes, D, true);
  if (p.ws_stride < need)
    return fail(VCMI_ERR_ARG, "BlockDiagTrajectoryGVGMMMap: workspace of %lld doubles below %lld", (long long)p.ws_stride,
                (long long)need);
  const int nres = gvp_resident(D, p.Tmax);
  const size_t shmem = gvp_lds_bytes(D, p.Tmax);
  auto kern = nres == 6 ? traj_gvp_kernel<6> : nres == 5 ? traj_gvp_kernel<5> : nres == 4 ? traj_gvp_kernel<4>
            : nres == 3 ? traj_gvp_kernel<3> : nres == 2 ? traj_gvp_kernel<2> : traj_gvp_kernel<0>;
  VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(kern, dim3(p.grid), dim3(kGvdThreads), shmem, st, p.du, p.n, D, (int64_t)p.Tmax * D, t->dg_q.p, t->mhat.p, t->gbuf.p,
                     t->ws.p, p.nframes, gv);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

}  // namespace vcmi
