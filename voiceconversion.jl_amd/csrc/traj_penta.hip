// traj_penta.hip -- trajectory conversion with THREE windows (static + delta + delta-delta) over diagonal conditional precisions:
// the solver of a handle of vcmi_traj_create_bdiag_windows(b, T, 3) (include/vcmi.h).
//
// With a delta-delta window the even and odd frames of traj_diag.hip no longer decouple: per utterance and static dimension the
// normal equations are ONE symmetric pentadiagonal system over all frames, positive definite and not diagonally dominant.
// Statement, the L D L' recurrence and its per-step arithmetic: traj_penta_step.hpp (shared with the host check).  Here: the
// kernel around those steps and its launch; the workspace rule: traj_band_plan.hpp.
#include "traj_internal.hpp"
#include "traj_band_plan.hpp"
#include "traj_penta_step.hpp"

namespace vcmi {

// steps whose loads are in flight ahead of the one the chain is at (two rings in the forward sweep, as in traj_diag.hip: mhat,
// then what it indexes).  A forward step issues 7 loads (mhat of a frame; its three precisions and three g) and 3 stores
// (l1, l2, z/d): 60 memory operations in flight at six steps, under the 63 the wave's counter holds (seven steps would be 70).
static constexpr int kPentaRing = 6;

// ------------------------------------------------------------------------------------------------
// One wave per (utterance, slab of 64 static dimensions): lane = dimension, every lane runs the chain over all T frames of its
// dimension.  No LDS, no barrier, no cross-lane traffic, no atomics.  Every access of the wave is up to 64 consecutive doubles
// of a (frame, 3D) row (of a (frame, D) row for Y and the two workspace arrays).
// Forward, step t: penta_forward_step on the carried rows of frames t-1 and t and the ring's row of frame t+1;
//   l1[t], l2[t] -> workspace, z[t] / d[t] -> Y;   backward, in place:  y[t] = Y[t] - l1[t] y[t+1] - l2[t] y[t+2].
// Lanes past D in the last slab and steps past the end of the utterance (the loops run in whole rings) work on clamped addresses
// and store nothing: EXEC stays full outside the stores.  A step past the end keeps p_s of the last frame in its pivot, so
// nothing there divides by zero; what it computes is never stored and never read.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
traj_penta_solve_kernel(const TrajUtt *__restrict__ utts, int nslab, int D, const double *__restrict__ q,
                        const int64_t *__restrict__ mhat_all, const double *__restrict__ g_all, double *__restrict__ l1_all,
                        double *__restrict__ l2_all) {
  constexpr int R = kPentaRing;
  const int u = (int)(blockIdx.x / (unsigned)nslab), slab = (int)(blockIdx.x % (unsigned)nslab);
  const TrajUtt U = utts[u];
  const int T = U.T;
  if (T == 0) return;
  const int D3 = 3 * D, lane = threadIdx.x;
  const int d0 = slab * kPentaSlab + lane;
  const bool live = d0 < D;
  const int d = live ? d0 : D - 1;
  const int64_t *mh = mhat_all + U.frame0;
  const int *mh32 = reinterpret_cast<const int *>(mh);     // the LOW word alone (1 <= mhat <= M), as traj_diag_solve_kernel
  const double *g = g_all + U.frame0 * D3;
  double *w1 = l1_all + U.frame0 * D, *w2 = l2_all + U.frame0 * D;
  gdouble *Y = (gdouble *)U.Y;
  const int Tl = T - 1;

  // the mixture of frame f (clamped to the utterance), 1-based as stored ...
  auto load_mix = [&](int f, int &m) { m = mh32[2 * (size_t)(f < Tl ? f : Tl)]; };
  // ... and through it the row of frame f
  auto load_row = [&](int f, int m, PentaRow &r) {
    const size_t fc = (size_t)(f < Tl ? f : Tl);
    const double *qm = q + (size_t)(m - 1) * D3 + d, *gf = g + fc * D3 + d;
    r.ps = qm[0];
    r.pd = qm[D];
    r.pa = qm[2 * D];
    r.gs = gf[0];
    r.gd = gf[D];
    r.ga = gf[2 * D];
  };

  // slot j of the rings holds frame k + 1 of the step k = kb + j that consumes it
  int mr[R];
  PentaRow rr[R];
#pragma unroll
  for (int j = 0; j < R; ++j) load_mix(j + 1, mr[j]);
  PentaFwd s;
  {
    int m0;
    load_mix(0, m0);
    load_row(0, m0, s.cur);
  }
#pragma unroll
  for (int j = 0; j < R; ++j) load_row(j + 1, mr[j], rr[j]);
#pragma unroll
  for (int j = 0; j < R; ++j) load_mix(R + j + 1, mr[j]);

  for (int kb = 0; kb < T; kb += R) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int t = kb + j;
      double l1, l2, zd;
      penta_forward_step(s, rr[j], t, T, l1, l2, zd);
      if (live && t < T) {
        w1[(size_t)t * D + d] = l1;
        w2[(size_t)t * D + d] = l2;
        Y[(size_t)t * D + d] = zd;
      }
      // the slots of the step just done take the loads of steps t + R and t + 2R, issued after their last use
      load_row(t + 1 + R, mr[j], rr[j]);
      load_mix(t + 1 + 2 * R, mr[j]);
    }
  }

  // back substitution from the last frame; the ring holds z/d, l1, l2 of the R steps below the current one
  const int Tr = (T + R - 1) / R * R;
  auto load_back = [&](int t, double &zd, double &l1, double &l2) {
    int tc = t > 0 ? t : 0;
    tc = tc < Tl ? tc : Tl;
    zd = Y[(size_t)tc * D + d];
    l1 = w1[(size_t)tc * D + d];
    l2 = w2[(size_t)tc * D + d];
  };
  double zr[R], l1r[R], l2r[R];
#pragma unroll
  for (int j = 0; j < R; ++j) load_back(Tr - 1 - j, zr[j], l1r[j], l2r[j]);
  double y1 = 0.0, y2 = 0.0;
  for (int kb = Tr - 1; kb >= 0; kb -= R) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int t = kb - j;
      const bool on = t < T;                         // (steps past the end leave y[t+1] = y[t+2] = 0)
      const double y = on ? penta_backward_step(zr[j], l1r[j], l2r[j], y1, y2) : 0.0;
      y2 = y1;
      y1 = y;
      if (live && on) Y[(size_t)t * D + d] = y;
      load_back(t - R, zr[j], l1r[j], l2r[j]);
    }
  }
}

int traj_penta_launch(vcmi_traj *t, const TrajSolvePlan &p, const double *q, const int64_t *mh, hipStream_t st) {
  const int nslab = penta_slabs(t->D);
  double *ws = t->ws.p;
  hipLaunchKernelGGL(traj_penta_solve_kernel, dim3((unsigned)((int64_t)p.n * nslab)), dim3(64), 0, st, p.du, nslab, t->D, q, mh,
                     t->gbuf.p, ws + penta_l1_offset(p.nframes, t->D), ws + penta_l2_offset(p.nframes, t->D));
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

}  // namespace vcmi
