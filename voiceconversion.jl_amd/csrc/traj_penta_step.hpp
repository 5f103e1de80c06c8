// traj_penta_step.hpp -- the per-step arithmetic of the pentadiagonal solver (traj_penta.hip: three windows, static + delta +
// delta-delta, over diagonal conditional precisions).  Compiles for the device and for the HOST: tests/c/traj_penta_check.cpp
// runs the same steps on the CPU, with 1.0 / x in place of the hardware seed of the reciprocal.  No memory access, no HIP call.
//
// Per utterance and static dimension the normal equations P y = r are symmetric pentadiagonal (rows [static; delta; delta-delta],
// the delta row of frame t holds -1/2 at t-1 and +1/2 at t+1, the delta-delta row 1, -2, 1; entries outside the utterance are
// dropped, the -2 is always there).  With q[mhat_t] = [p_s(t); p_d(t); p_a(t)] and g_t = [g_s; g_d; g_a]:
//   P[t,t]   = p_s(t) + p_d(t-1)/4 + p_d(t+1)/4 + p_a(t-1) + 4 p_a(t) + p_a(t+1)
//   P[t,t+1] = -2 p_a(t) - 2 p_a(t+1)                      (t+1 < T)
//   P[t,t+2] = -p_d(t+1)/4 + p_a(t+1)                      (t+2 < T)
//   r[t]     = g_s(t) + g_d(t-1)/2 - g_d(t+1)/2 + g_a(t-1) - 2 g_a(t) + g_a(t+1)
// P = diag(p_s) + (a Gram matrix): symmetric positive definite for p_s > 0, NOT diagonally dominant.  The solve is
// P = L D L' without pivoting (backward stable on such matrices), L unit lower triangular with the two subdiagonals l1, l2:
//   d[t]  = P[t,t] - l1[t-1]^2 d[t-1] - l2[t-2]^2 d[t-2]
//   l1[t] = (P[t,t+1] - l2[t-1] l1[t-1] d[t-1]) / d[t]        l2[t] = P[t,t+2] / d[t]
//   z[t]  = r[t] - l1[t-1] z[t-1] - l2[t-2] z[t-2]            y[t]  = z[t] / d[t] - l1[t] y[t+1] - l2[t] y[t+2]   (backward)
// carried in the numerators c1[t] = l1[t] d[t], c2[t] = l2[t] d[t], so that l^2 d = l c needs no square and the chain from one
// pivot to the next is one multiply (l1 = c1 / d), one fma and the reciprocal.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define VCMI_PENTA_HD __host__ __device__ __forceinline__
#else
#define VCMI_PENTA_HD inline
#endif

namespace vcmi {

// 1/x in FP64, traj_rcp's arithmetic (traj_diag.hip): seed + two Newton steps.  x is a pivot: positive, finite.
VCMI_PENTA_HD double penta_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  double y = __builtin_amdgcn_rcp(x);
#else
  double y = 1.0 / x;
#endif
  y = fma(fma(-x, y, 1.0), y, y);
  y = fma(fma(-x, y, 1.0), y, y);
  return y;
}

// q[mhat_t] and g_t of one frame at one static dimension
struct PentaRow {
  double ps, pd, pa, gs, gd, ga;
};

// what the forward sweep carries from step to step; all zero in front of frame 0 except `cur`, the row of frame 0
struct PentaFwd {
  PentaRow cur;                                      // frame t (delta and delta-delta parts zero when t >= T)
  double pdp = 0.0, pap = 0.0, gdp = 0.0, gap = 0.0;   // frame t-1
  double l1p = 0.0, c1p = 0.0;                         // l1[t-1], c1[t-1]
  double l2p = 0.0, c2p = 0.0;                         // l2[t-1], c2[t-1]
  double l2pp = 0.0, s2 = 0.0;                         // l2[t-2], l2[t-2] c2[t-2]
  double zp = 0.0, zpp = 0.0;                          // z[t-1], z[t-2]
};

// Forward step at frame t of T: `nx` is the row of frame t+1 AS LOADED (from a clamped address when t+1 >= T: its delta and
// delta-delta parts are dropped here; p_s and g_s stay, which keeps the pivot of a step past the end positive).
// Out: l1[t], l2[t] and z[t] / d[t], what the back substitution reads.
VCMI_PENTA_HD void penta_forward_step(PentaFwd &s, const PentaRow &nx, int t, int T, double &l1, double &l2, double &zd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool h1 = t + 1 < T, h2 = t + 2 < T;
  const double pdn = h1 ? nx.pd : 0.0, pan = h1 ? nx.pa : 0.0, gdn = h1 ? nx.gd : 0.0, gan = h1 ? nx.ga : 0.0;
  const PentaRow &c = s.cur;
  const double ptt = c.ps + 0.25 * s.pdp + 0.25 * pdn + s.pap + 4.0 * c.pa + pan;
  const double p1 = h1 ? -2.0 * c.pa - 2.0 * pan : 0.0;
  const double p2 = h2 ? -0.25 * pdn + pan : 0.0;
  const double r = c.gs + 0.5 * s.gdp - 0.5 * gdn + s.gap - 2.0 * c.ga + gan;
  // the chain: l1p (one multiply behind the last reciprocal) -> d -> 1/d
  const double d = fma(-s.l1p, s.c1p, ptt - s.s2);
  const double rd = penta_rcp(d);
  const double c1 = fma(-s.l2p, s.c1p, p1);
  const double z = fma(-s.l1p, s.zp, fma(-s.l2pp, s.zpp, r));
  l1 = c1 * rd;
  l2 = p2 * rd;
  zd = z * rd;
  s.s2 = s.l2p * s.c2p;
  s.l2pp = s.l2p;
  s.zpp = s.zp;
  s.zp = z;
  s.l1p = l1;
  s.c1p = c1;
  s.l2p = l2;
  s.c2p = p2;
  s.pdp = c.pd;
  s.pap = c.pa;
  s.gdp = c.gd;
  s.gap = c.ga;
  s.cur = PentaRow{nx.ps, pdn, pan, nx.gs, gdn, gan};
}

// Backward step: y[t] from z[t] / d[t], l1[t], l2[t] and the two solutions above (zero past the end)
VCMI_PENTA_HD double penta_backward_step(double zd, double l1, double l2, double y1, double y2) {
  return fma(-l2, y2, fma(-l1, y1, zd));
}

}  // namespace vcmi
