// traj_gv_band_step.hpp -- the per-element arithmetic of the global-variance ascents over diagonal conditional precisions
// (traj_gv_band.hip: traj_gvd_kernel over two windows, traj_gvp_kernel over three).  Compiles for the device and for the HOST:
// tests/c/traj_gvp_check.cpp runs the same text on the CPU against a long-double evaluation.  No memory access, no HIP call.
//
// Notation of traj_penta_step.hpp: q[mhat_t] = [p_s(t); p_d(t); p_a(t)], g_t = [g_s; g_d; g_a] (two windows: no p_a, no g_a); P and
// r per static dimension are the matrix and the right-hand side that the solver of the handle factorises (traj_diag_solve_kernel,
// traj_penta_solve_kernel), stored by COLUMN t as the epoch reads them:
//   c0_t = P[t,t]   = p_s(t) + p_d(t-1)/4 + p_d(t+1)/4 + p_a(t-1) + 4 p_a(t) + p_a(t+1)
//   c1_t = P[t-1,t] = -2 p_a(t-1) - 2 p_a(t)                 (0 for t < 1; three windows only)
//   c2_t = P[t-2,t] = -p_d(t-1)/4 + p_a(t-1)                 (0 for t < 2)
//   r_t  = g_s(t) + g_d(t-1)/2 - g_d(t+1)/2 + g_a(t-1) - 2 g_a(t) + g_a(t+1)
//   (P y)_t = c0_t y_t + c1_t y_{t-1} + c1_{t+1} y_{t+1} + c2_t y_{t-2} + c2_{t+2} y_{t+2}
// A p or g of a frame outside the utterance is absent; a y_{t+-1}, y_{t+-2} outside the utterance gets weight 0 while what the
// existing neighbour frames add to c0 stays.  The epoch is the reference's (src/trajectory_gmmmap.jl:163-166, eq. (52)):
//   y_t <- y_t + alpha ( omega (r_t - (P y)_t) + coef (y_t - mean) ),    omega = 1/(2T),  coef = -2/T pv' (var_1(y) - mu_v)
// Contraction is off: what is fused is written as fma.
#pragma once
#include <cmath>

#include "traj_penta_step.hpp"

namespace vcmi {

// ---- two windows ----
struct GvdCoef {
  double c0, c2, r;
};

// The three stored values of frame t of T from p_s(t), g_s(t) and the p_d, g_d of frames t-1 (pdm, gdm) and t+1 (pdp, gdp) AS
// LOADED (from clamped addresses where the frame does not exist: its parts get weight 0 here).
VCMI_PENTA_HD GvdCoef gvd_coefficients(double ps, double pdm, double pdp, double gs, double gdm, double gdp, int t, int T) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  GvdCoef o;
  o.r = (gs + (t >= 1 ? 0.5 : 0.0) * gdm) - (t + 1 < T ? 0.5 : 0.0) * gdp;
  o.c0 = (ps + (t >= 1 ? 0.25 : 0.0) * pdm) + (t + 1 < T ? 0.25 : 0.0) * pdp;
  o.c2 = t >= 2 ? -0.25 * pdm : 0.0;
  return o;
}

// One element of one epoch.  y0 = y_t, ym2 / yp2 its neighbours and c2n = c2_{t+2} AS LOADED (clamped addresses: what lies past
// the end gets weight 0 here; c2_t is stored as 0 where y_{t-2} does not exist).
VCMI_PENTA_HD double gvd_epoch_step(double y0, double ym2, double yp2, double c0, double c2, double c2n, double r, int t, int T,
                                    double omega, double coef, double mean, double alpha) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double w2 = t + 2 < T ? c2n : 0.0;
  const double py = fma(w2, yp2, fma(c2, ym2, c0 * y0));
  const double dy = fma(coef, y0 - mean, omega * (r - py));
  return fma(alpha, dy, y0);
}

// ---- three windows ----
struct GvpCoef {
  double c0, c1, c2, r;
};

// The four stored values of frame t of T from the rows of frames t-1, t, t+1 AS LOADED (from clamped addresses where the frame
// does not exist: its parts are dropped here).  c0 and r are summed in the order of penta_forward_step: for the same rows they
// are the solver's P[t,t] and r[t] bit for bit.
VCMI_PENTA_HD GvpCoef gvp_coefficients(const PentaRow &pv, const PentaRow &c, const PentaRow &nx, int t, int T) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool hm = t >= 1, hp = t + 1 < T;
  const double pdp = hm ? pv.pd : 0.0, pap = hm ? pv.pa : 0.0, gdp = hm ? pv.gd : 0.0, gap = hm ? pv.ga : 0.0;
  const double pdn = hp ? nx.pd : 0.0, pan = hp ? nx.pa : 0.0, gdn = hp ? nx.gd : 0.0, gan = hp ? nx.ga : 0.0;
  GvpCoef o;
  o.c0 = c.ps + 0.25 * pdp + 0.25 * pdn + pap + 4.0 * c.pa + pan;
  o.c1 = hm ? -2.0 * pap - 2.0 * c.pa : 0.0;
  o.c2 = t >= 2 ? -0.25 * pdp + pap : 0.0;
  o.r = c.gs + 0.5 * gdp - 0.5 * gdn + gap - 2.0 * c.ga + gan;
  return o;
}

// One element of one epoch.  y0 = y_t, ym1 / yp1 / ym2 / yp2 its neighbours and c1n = c1_{t+1}, c2n = c2_{t+2} AS LOADED (clamped
// addresses: what lies past the end gets weight 0 here; c1_t and c2_t are stored as 0 where y_{t-1} / y_{t-2} do not exist).
VCMI_PENTA_HD double gvp_epoch_step(double y0, double ym1, double yp1, double ym2, double yp2, double c0, double c1, double c1n,
                                    double c2, double c2n, double r, int t, int T, double omega, double coef, double mean,
                                    double alpha) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double w1 = t + 1 < T ? c1n : 0.0, w2 = t + 2 < T ? c2n : 0.0;
  const double py = fma(w2, yp2, fma(c2, ym2, fma(w1, yp1, fma(c1, ym1, c0 * y0))));
  const double dy = fma(coef, y0 - mean, omega * (r - py));
  return fma(alpha, dy, y0);
}

}  // namespace vcmi
