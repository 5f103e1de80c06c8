// traj_gvp_check.cpp -- the per-element arithmetic of the GV ascents over diagonal conditional precisions (csrc/traj_gv_band_step.hpp,
// the header the kernels of csrc/traj_gv_band.hip are made of, compiled here for the HOST) and the launch rule of the three-window
// one (csrc/traj_band_plan.hpp) on the CPU.
//   1. Chains of T = 2, 3, 4, 5, 50, 2000 frames, precisions spread over five decades: the coefficients and a run of Jacobi epochs
//      driven as the kernel drives them (neighbour rows and neighbour y from addresses clamped into the utterance, two y buffers)
//      against a long-double evaluation of the assembled pentadiagonal P and r at the chain's own y_n, element by element within
//      K 2^-53 (|y| + |y'| + alpha (omega (r_abs + |P||y|) + |coef||y - mean|)), K = 16: eleven terms in r - P y, the update.
//   1b. The same chains through the two-window step (gvd_coefficients, gvd_epoch_step) against the assembled tridiagonal-in-
//      parity P and r, within the same bar with K = 8 (chains2 says how the roundings are counted).
//   2. The rule's invariants: never above the LDS limit, monotone in T, fewer than two arrays resident means none, the workspace
//      covers the five arrays the kernel writes for every utterance of a call and lies on l1 / l2 without exceeding the reserve;
//      and the table of (D, T, resident) lines that tests/test_gv_penta_restatement_host.py compares with the Python restatement.
// Built by tests/test_gv_penta_restatement_host.py with -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../voiceconversion.jl_amd/csrc/traj_band_plan.hpp"
#include "../../voiceconversion.jl_amd/csrc/traj_gv_band_step.hpp"

using namespace vcmi;
typedef long double ld;

static int bad = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      if (++bad <= 20) printf("traj_gvp_check: %s (line %d)\n", #cond, __LINE__);        \
    }                                                                                    \
  } while (0)

static const double kEps = std::ldexp(1.0, -53);

static void chains() {
  static const int Ts[] = {2, 3, 4, 5, 50, 2000};
  std::mt19937_64 rng(20240611);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::normal_distribution<double> gauss(0.0, 1.0);
  double worst = 0.0;
  for (int T : Ts) {
    for (int rep = 0; rep < 4; ++rep) {
      std::vector<PentaRow> rows(T);
      const double ls = -2.0 + 3.0 * u(rng), ldl = -2.0 + 3.0 * u(rng), la = -2.0 + 3.0 * u(rng);
      for (int t = 0; t < T; ++t) {
        PentaRow &c = rows[t];
        c.ps = std::pow(10.0, ls + 2.0 * u(rng));
        c.pd = std::pow(10.0, ldl + 2.0 * u(rng));
        c.pa = std::pow(10.0, la + 2.0 * u(rng));
        c.gs = c.ps * (std::sin(0.05 * t) + 0.3 * gauss(rng));
        c.gd = c.pd * 0.1 * gauss(rng);
        c.ga = c.pa * 0.05 * gauss(rng);
      }
      // the prologue: rows of frames t-1 and t+1 from clamped addresses
      std::vector<double> c0(T), c1(T), c2(T), r(T);
      std::vector<ld> L0(T), L1(T, 0.0L), L2(T, 0.0L), L2m(T, 0.0L), Lr(T), Lra(T);
      for (int t = 0; t < T; ++t) {
        const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
        const GvpCoef k = gvp_coefficients(rows[tm], rows[t], rows[tp], t, T);
        c0[t] = k.c0, c1[t] = k.c1, c2[t] = k.c2, r[t] = k.r;
        const PentaRow &c = rows[t];
        ld d = (ld)c.ps + 4.0L * c.pa, v = (ld)c.gs - 2.0L * c.ga, va = fabsl((ld)c.gs) + 2.0L * fabsl((ld)c.ga);
        if (t >= 1) {
          const PentaRow &m = rows[t - 1];
          d += 0.25L * m.pd + m.pa;
          v += 0.5L * m.gd + m.ga;
          va += 0.5L * fabsl((ld)m.gd) + fabsl((ld)m.ga);
          L1[t] = -2.0L * m.pa - 2.0L * c.pa;
          if (t >= 2) L2[t] = -0.25L * m.pd + m.pa, L2m[t] = 0.25L * m.pd + m.pa;
        }
        if (t + 1 < T) {
          const PentaRow &n = rows[t + 1];
          d += 0.25L * n.pd + n.pa;
          v += -0.5L * n.gd + n.ga;
          va += 0.5L * fabsl((ld)n.gd) + fabsl((ld)n.ga);
        }
        L0[t] = d, Lr[t] = v, Lra[t] = va;
        CHECK(fabsl((ld)k.c0 - d) <= 8 * kEps * d && fabsl((ld)k.c1 - L1[t]) <= 4 * kEps * fabsl(L1[t]));
        CHECK(fabsl((ld)k.c2 - L2[t]) <= 4 * kEps * L2m[t] && fabsl((ld)k.r - v) <= 8 * kEps * va);
        CHECK((t >= 1 || k.c1 == 0.0) && (t >= 2 || k.c2 == 0.0));
      }
      // epochs: Jacobi on two buffers, every load on a clamped address
      const double omega = 1.0 / (2.0 * T), alpha = 0.3 / (double)(L0[0] * omega), coef = -0.01 * (double)L0[0] * omega;
      std::vector<double> y(T), yn(T);
      for (int t = 0; t < T; ++t) y[t] = std::sin(0.05 * t) + 0.3 * gauss(rng);
      for (int ep = 0; ep < 5; ++ep) {
        double mean = 0.0;
        for (int t = 0; t < T; ++t) mean += y[t];
        mean /= T;
        for (int t = 0; t < T; ++t) {
          const int t1m = t >= 1 ? t - 1 : t, t1p = t + 1 < T ? t + 1 : t, t2m = t >= 2 ? t - 2 : t, t2p = t + 2 < T ? t + 2 : t;
          yn[t] = gvp_epoch_step(y[t], y[t1m], y[t1p], y[t2m], y[t2p], c0[t], c1[t], c1[t1p], c2[t], c2[t2p], r[t], t, T, omega, coef,
                                 mean, alpha);
          ld py = L0[t] * y[t], pa = L0[t] * fabsl((ld)y[t]);
          if (t >= 1) py += L1[t] * y[t - 1], pa += fabsl(L1[t] * y[t - 1]);
          if (t + 1 < T) py += L1[t + 1] * y[t + 1], pa += fabsl(L1[t + 1] * y[t + 1]);
          if (t >= 2) py += L2[t] * y[t - 2], pa += L2m[t] * fabsl((ld)y[t - 2]);
          if (t + 2 < T) py += L2[t + 2] * y[t + 2], pa += L2m[t + 2] * fabsl((ld)y[t + 2]);
          const ld ref = (ld)y[t] + (ld)alpha * ((ld)omega * (Lr[t] - py) + (ld)coef * ((ld)y[t] - (ld)mean));
          const ld mag = fabsl((ld)y[t]) + fabsl(ref) +
                         (ld)alpha * ((ld)omega * (Lra[t] + pa) + fabsl((ld)coef) * (fabsl((ld)y[t]) + fabsl((ld)mean)));
          const double ratio = (double)(fabsl((ld)yn[t] - ref) / (16 * kEps * mag));
          CHECK(std::isfinite(yn[t]) && ratio <= 1.0);
          if (ratio > worst) worst = ratio;
        }
        y.swap(yn);
      }
      printf("chain T %d rep %d: worst error / bar so far %.3e\n", T, rep, worst);
    }
  }
}

// The two-window step, driven as traj_gvd_kernel drives it.  The bar is that of chains() with K counted for this stencil, to
// first order in u = 2^-53, every rounding relative to a sum of magnitudes that the bar holds (multiplications by 0.25 and 0.5
// are exact, so c2 is exact; omega, coef, mean and alpha are the same doubles on both sides):
//   r        2 additions                                              2 u r_abs
//   P y      c0: 2 additions; c0 y; the two fma                       5 u |P||y|
//   r - P y  1 subtraction                     -> at most 6 u (r_abs + |P||y|)
//   omega .  1 multiplication                  -> 7 u omega (r_abs + |P||y|)
//   y - mean 1 subtraction, then the fma       -> 8 u omega (r_abs + |P||y|) + 2 u |coef| (|y| + |mean|)
//   the last fma                               -> + u |y'|
// so K = 8 (the three-window step has 5 roundings in r, 10 in P y and the same 3 behind them: 13, hence its 16).  The stored
// coefficients: c0 and r within 3 u of their magnitude sums (two roundings and the long-double sum's own), c2 exactly.
static void chains2() {
  static const int Ts[] = {2, 3, 4, 5, 50, 2000};
  std::mt19937_64 rng(20240612);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::normal_distribution<double> gauss(0.0, 1.0);
  double worst = 0.0;
  for (int T : Ts) {
    for (int rep = 0; rep < 4; ++rep) {
      std::vector<double> ps(T), pd(T), gs(T), gd(T);
      const double ls = -2.0 + 3.0 * u(rng), ldl = -2.0 + 3.0 * u(rng);
      for (int t = 0; t < T; ++t) {
        ps[t] = std::pow(10.0, ls + 2.0 * u(rng));
        pd[t] = std::pow(10.0, ldl + 2.0 * u(rng));
        gs[t] = ps[t] * (std::sin(0.05 * t) + 0.3 * gauss(rng));
        gd[t] = pd[t] * 0.1 * gauss(rng);
      }
      // the prologue: p_d and g_d of frames t-1 and t+1 from clamped addresses
      std::vector<double> c0(T), c2(T), r(T);
      std::vector<ld> L0(T), L2(T, 0.0L), Lr(T), Lra(T);
      for (int t = 0; t < T; ++t) {
        const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
        const GvdCoef k = gvd_coefficients(ps[t], pd[tm], pd[tp], gs[t], gd[tm], gd[tp], t, T);
        c0[t] = k.c0, c2[t] = k.c2, r[t] = k.r;
        ld d = (ld)ps[t], v = (ld)gs[t], va = fabsl((ld)gs[t]);
        if (t >= 1) {
          d += 0.25L * pd[t - 1];
          v += 0.5L * gd[t - 1];
          va += 0.5L * fabsl((ld)gd[t - 1]);
          if (t >= 2) L2[t] = -0.25L * pd[t - 1];
        }
        if (t + 1 < T) {
          d += 0.25L * pd[t + 1];
          v -= 0.5L * gd[t + 1];
          va += 0.5L * fabsl((ld)gd[t + 1]);
        }
        L0[t] = d, Lr[t] = v, Lra[t] = va;
        CHECK(fabsl((ld)k.c0 - d) <= 3 * kEps * d && fabsl((ld)k.r - v) <= 3 * kEps * va);
        CHECK((ld)k.c2 == L2[t] && (t >= 2 || k.c2 == 0.0));
      }
      // epochs: Jacobi on two buffers, every load on a clamped address
      const double omega = 1.0 / (2.0 * T), alpha = 0.3 / (double)(L0[0] * omega), coef = -0.01 * (double)L0[0] * omega;
      std::vector<double> y(T), yn(T);
      for (int t = 0; t < T; ++t) y[t] = std::sin(0.05 * t) + 0.3 * gauss(rng);
      for (int ep = 0; ep < 5; ++ep) {
        double mean = 0.0;
        for (int t = 0; t < T; ++t) mean += y[t];
        mean /= T;
        for (int t = 0; t < T; ++t) {
          const int t2m = t >= 2 ? t - 2 : t, t2p = t + 2 < T ? t + 2 : t;
          yn[t] = gvd_epoch_step(y[t], y[t2m], y[t2p], c0[t], c2[t], c2[t2p], r[t], t, T, omega, coef, mean, alpha);
          ld py = L0[t] * y[t], pa = L0[t] * fabsl((ld)y[t]);
          if (t >= 2) py += L2[t] * y[t - 2], pa += fabsl(L2[t] * y[t - 2]);
          if (t + 2 < T) py += L2[t + 2] * y[t + 2], pa += fabsl(L2[t + 2] * y[t + 2]);
          const ld ref = (ld)y[t] + (ld)alpha * ((ld)omega * (Lr[t] - py) + (ld)coef * ((ld)y[t] - (ld)mean));
          const ld mag = fabsl((ld)y[t]) + fabsl(ref) +
                         (ld)alpha * ((ld)omega * (Lra[t] + pa) + fabsl((ld)coef) * (fabsl((ld)y[t]) + fabsl((ld)mean)));
          const double ratio = (double)(fabsl((ld)yn[t] - ref) / (8 * kEps * mag));
          CHECK(std::isfinite(yn[t]) && ratio <= 1.0);
          if (ratio > worst) worst = ratio;
        }
        y.swap(yn);
      }
      printf("two-window chain T %d rep %d: worst error / bar so far %.3e\n", T, rep, worst);
    }
  }
}

static void plan() {
  static const int64_t Ns[] = {0, 1, 2, 70, 1000, 512000, (int64_t)1 << 31};
  CHECK(kGvpArrays == 6 && kGvpWsArrays == 5);
  for (int D = 1; D <= 128; ++D) {
    int prev = kGvpArrays;
    for (int64_t T = 1; T <= 6000; ++T) {
      const int n = gvp_resident(D, T);
      CHECK(n == 0 || (n >= 2 && n <= kGvpArrays));
      CHECK(n <= prev);                                                     // monotone: a longer utterance never keeps more
      CHECK(gvp_lds_bytes(D, T) <= kGvdLdsLimit);
      CHECK(gvp_lds_bytes(D, T) == gvp_fixed_lds_bytes(D) + (size_t)n * T * D * 8);
      if (n < kGvpArrays && n > 0) CHECK(gvp_fixed_lds_bytes(D) + (size_t)(n + 1) * T * D * 8 > kGvdLdsLimit);   // as many as fit
      if (n == 0) CHECK(gvp_fixed_lds_bytes(D) + (size_t)2 * T * D * 8 > kGvdLdsLimit);
      prev = n;
    }
    CHECK(gvp_resident(D, 0) == 0 && gvp_resident(D, (int64_t)1 << 31) == 0);
    for (int64_t n : Ns) {
      const int64_t ws = gvp_ws_doubles(n, D, true), one = n * D;
      CHECK(ws == 5 * one && gvp_ws_doubles(n, D, false) == penta_ws_doubles(n, D) && ws >= penta_ws_doubles(n, D));
      // the second y lies on l1, c1 on l2; every array inside the reserve, none overlapping the next
      CHECK(gvp_ws_offset(0, n, D) == penta_l1_offset(n, D) && gvp_ws_offset(1, n, D) == penta_l2_offset(n, D));
      for (int k = 0; k < kGvpWsArrays; ++k) CHECK(gvp_ws_offset(k, n, D) + one <= (k + 1 < kGvpWsArrays ? gvp_ws_offset(k + 1, n, D) : ws));
      // what the kernel writes for an utterance of T frames at frame0: [offset + frame0 D, offset + (frame0 + T) D)
      if (n >= 2) {
        const int64_t T = n / 2, frame0 = n - T;
        CHECK(gvp_ws_offset(kGvpWsArrays - 1, n, D) + (frame0 + T) * D <= ws);
      }
    }
  }
  CHECK(gvp_ws_doubles((int64_t)1 << 31, 128, true) == ((int64_t)5 << 38));
  // the table the Python restatement is compared with
  static const int Dt[] = {1, 4, 12, 33, 40, 42, 128};
  static const int64_t Tt[] = {1, 2, 50, 100, 269, 270, 323, 324, 403, 404, 538, 539, 807, 808, 2000, 100000};
  for (int D : Dt)
    for (int64_t T : Tt) printf("resident D %d T %lld : %d\n", D, (long long)T, gvp_resident(D, T));
}

int main() {
  chains();
  chains2();
  plan();
  if (bad) {
    printf("traj_gvp_check: %d failures\n", bad);
    return 1;
  }
  printf("traj_gvp_check: ok\n");
  return 0;
}
