// traj_penta_check.cpp -- the pentadiagonal solver's per-step arithmetic (csrc/traj_penta_step.hpp, the header the kernel of
// csrc/traj_penta.hip is made of, compiled here for the HOST: 1.0 / x in place of the hardware seed) and its workspace rule
// (csrc/traj_band_plan.hpp) on the CPU.
//   1. Chains of T = 1, 2, 3, 4, 5, 50, 2000 frames, precisions spread over five decades: the forward and backward steps, driven
//      as the kernel drives them (rows of frames past the end taken from the last frame, whole rings of six steps, nothing of a
//      step past the end stored), against a long-double solve of the explicitly assembled matrix (Gaussian elimination on the
//      dense matrix in long double; for T = 2000 the loops skip what lies outside the band, which stays zero), within
//      relerr < 64 cond rho 2^-53 -- cond = lambda_max / lambda_min from power and inverse iteration in long double (both approach
//      from inside, so the bound used is not above the true one), rho = ||r_abs||_inf / ||r||_inf.
//   2. The plan's invariants: the workspace covers two arrays, l2 lies behind l1 without overlap, and a two-window plan is
//      gvd_ws_doubles exactly for every D up to 128.
// Built by tests/test_traj_penta_host.py with -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../voiceconversion.jl_amd/csrc/traj_band_plan.hpp"
#include "../../voiceconversion.jl_amd/csrc/traj_penta_step.hpp"

using namespace vcmi;
typedef long double ld;

static int bad = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      if (++bad <= 20) printf("traj_penta_check: %s (line %d)\n", #cond, __LINE__);        \
    }                                                                                      \
  } while (0)

// the steps as traj_penta_solve_kernel runs them, one chain
static std::vector<double> solve_steps(const std::vector<PentaRow> &rows) {
  const int T = (int)rows.size(), R = 6, Tl = T - 1, Tr = (T + R - 1) / R * R;
  std::vector<double> l1(T), l2(T), y(T);
  auto row = [&](int f) { return rows[(size_t)(f < Tl ? f : Tl)]; };
  PentaFwd s;
  s.cur = row(0);
  for (int t = 0; t < Tr; ++t) {
    double a, b, zd;
    penta_forward_step(s, row(t + 1), t, T, a, b, zd);
    CHECK(std::isfinite(a) && std::isfinite(b) && std::isfinite(zd));      // also past the end
    if (t < T) {
      l1[t] = a;
      l2[t] = b;
      y[t] = zd;
    }
  }
  double y1 = 0.0, y2 = 0.0;
  for (int t = Tr - 1; t >= 0; --t) {
    const int tc = t < Tl ? t : Tl;
    const double v = t < T ? penta_backward_step(y[tc], l1[tc], l2[tc], y1, y2) : 0.0;
    y2 = y1;
    y1 = v;
    if (t < T) y[t] = v;
  }
  return y;
}

// P (dense, row-major T x T) and r from the closed form, in long double; rabs: every stencil sign taken positive
static void assemble(const std::vector<PentaRow> &rows, std::vector<ld> &P, std::vector<ld> &r, std::vector<ld> &rabs) {
  const int T = (int)rows.size();
  P.assign((size_t)T * T, 0.0L);
  r.assign(T, 0.0L);
  rabs.assign(T, 0.0L);
  for (int t = 0; t < T; ++t) {
    const PentaRow &c = rows[t];
    ld d = (ld)c.ps + 4.0L * c.pa, v = (ld)c.gs - 2.0L * c.ga, va = fabsl((ld)c.gs) + 2.0L * fabsl((ld)c.ga);
    if (t >= 1) {
      const PentaRow &m = rows[t - 1];
      d += 0.25L * m.pd + m.pa;
      v += 0.5L * m.gd + m.ga;
      va += 0.5L * fabsl((ld)m.gd) + fabsl((ld)m.ga);
    }
    if (t + 1 < T) {
      const PentaRow &n = rows[t + 1];
      d += 0.25L * n.pd + n.pa;
      v += -0.5L * n.gd + n.ga;
      va += 0.5L * fabsl((ld)n.gd) + fabsl((ld)n.ga);
      P[(size_t)t * T + t + 1] = P[(size_t)(t + 1) * T + t] = -2.0L * c.pa - 2.0L * n.pa;
      if (t + 2 < T) P[(size_t)t * T + t + 2] = P[(size_t)(t + 2) * T + t] = -0.25L * n.pd + n.pa;
    }
    P[(size_t)t * T + t] = d;
    r[t] = v;
    rabs[t] = va;
  }
}

// Gaussian elimination without pivoting (P is symmetric positive definite) on the dense matrix, in place: the multipliers take
// the places of the entries they clear.  bw: how far from the diagonal the loops go (T - 1: everything)
static void factor_ld(std::vector<ld> &A, int T, int bw) {
  for (int k = 0; k < T; ++k) {
    const int hi = k + bw < T - 1 ? k + bw : T - 1;
    for (int i = k + 1; i <= hi; ++i) {
      const ld f = A[(size_t)i * T + k] / A[(size_t)k * T + k];
      A[(size_t)i * T + k] = f;
      if (f == 0.0L) continue;
      for (int j = k + 1; j <= hi; ++j) A[(size_t)i * T + j] -= f * A[(size_t)k * T + j];
    }
  }
}
static std::vector<ld> solve_ld(const std::vector<ld> &A, std::vector<ld> b, int T, int bw) {
  for (int k = 0; k < T; ++k) {
    const int hi = k + bw < T - 1 ? k + bw : T - 1;
    for (int i = k + 1; i <= hi; ++i) b[i] -= A[(size_t)i * T + k] * b[k];
  }
  for (int i = T - 1; i >= 0; --i) {
    const int hi = i + bw < T - 1 ? i + bw : T - 1;
    ld v = b[i];
    for (int j = i + 1; j <= hi; ++j) v -= A[(size_t)i * T + j] * b[j];
    b[i] = v / A[(size_t)i * T + i];
  }
  return b;
}

static ld norm2(const std::vector<ld> &v) {
  ld s = 0.0L;
  for (ld x : v) s += x * x;
  return sqrtl(s);
}

// lambda_max / lambda_min of the symmetric positive definite P: power iteration on P and, with its factors F, on its inverse
static double cond2(const std::vector<ld> &P, const std::vector<ld> &F, int T, int bw) {
  std::vector<ld> v(T), w(T);
  for (int i = 0; i < T; ++i) v[i] = 1.0L + 0.37L * ((i * 7919) % 13);
  ld lmax = 0.0L, imax = 0.0L;
  for (int it = 0; it < 300; ++it) {
    for (int i = 0; i < T; ++i) {
      ld s = 0.0L;
      const int lo = i - 2 > 0 ? i - 2 : 0, hi = i + 2 < T - 1 ? i + 2 : T - 1;
      for (int j = lo; j <= hi; ++j) s += P[(size_t)i * T + j] * v[j];
      w[i] = s;
    }
    lmax = norm2(w) / norm2(v);
    const ld n = norm2(w);
    for (int i = 0; i < T; ++i) v[i] = w[i] / n;
  }
  for (int i = 0; i < T; ++i) v[i] = 1.0L + 0.37L * ((i * 104729) % 11);
  for (int it = 0; it < 300; ++it) {
    w = solve_ld(F, v, T, bw);
    imax = norm2(w) / norm2(v);
    const ld n = norm2(w);
    for (int i = 0; i < T; ++i) v[i] = w[i] / n;
  }
  return (double)(lmax * imax);
}

static void chains() {
  static const int Ts[] = {1, 2, 3, 4, 5, 50, 2000};
  std::mt19937_64 rng(20240607);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::normal_distribution<double> gauss(0.0, 1.0);
  double worst = 0.0;
  for (int T : Ts) {
    const int reps = T >= 2000 ? 2 : 8;
    for (int rep = 0; rep < reps; ++rep) {
      // precisions over five decades, each block with its own level; g = p * (a smooth target + noise)
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
      std::vector<ld> P, r, rabs;
      assemble(rows, P, r, rabs);
      const int bw = T > 50 ? 2 : T - 1;
      std::vector<ld> F(P);
      factor_ld(F, T, bw);
      const std::vector<ld> ref = solve_ld(F, r, T, bw);
      const std::vector<double> y = solve_steps(rows);
      ld err = 0.0L, scale = 0.0L, rmax = 0.0L, ramax = 0.0L;
      for (int t = 0; t < T; ++t) {
        err = fmaxl(err, fabsl((ld)y[t] - ref[t]));
        scale = fmaxl(scale, fabsl(ref[t]));
        rmax = fmaxl(rmax, fabsl(r[t]));
        ramax = fmaxl(ramax, rabs[t]);
      }
      const double cond = T == 1 ? 1.0 : cond2(P, F, T, bw), rho = (double)(ramax / rmax);
      const double rel = (double)(err / scale), bound = 64.0 * cond * rho * std::ldexp(1.0, -53);
      printf("chain T %d rep %d: relerr %.3e cond %.3e rho %.3f bound %.3e ratio %.3e\n", T, rep, rel, cond, rho, bound, rel / bound);
      CHECK(cond >= 1.0 && rho >= 1.0 - 1e-12);
      CHECK(rel < bound);
      if (rel / bound > worst) worst = rel / bound;
    }
  }
  printf("worst relerr / bound: %.3e\n", worst);
}

static void plan() {
  static const int64_t Ns[] = {0, 1, 2, 70, 1000, 512000, (int64_t)1 << 31};
  for (int D = 1; D <= 128; ++D) {
    CHECK(penta_slabs(D) * kPentaSlab >= D && (penta_slabs(D) - 1) * kPentaSlab < D);
    for (int64_t n : Ns) {
      // two windows: the plan of the tridiagonal solver and of its GV ascent, unchanged
      CHECK(traj_diag_ws_doubles(2, n, D, false) == gvd_ws_doubles(n, D, false));
      CHECK(traj_diag_ws_doubles(2, n, D, true) == gvd_ws_doubles(n, D, true));
      // three windows: two (nframes, D) arrays, whatever with_gv says
      const int64_t ws = traj_diag_ws_doubles(3, n, D, false);
      CHECK(ws == penta_ws_doubles(n, D) && traj_diag_ws_doubles(3, n, D, true) == ws);
      CHECK(ws == 2 * n * D && kPentaArrays == 2);
      const int64_t o1 = penta_l1_offset(n, D), o2 = penta_l2_offset(n, D), one = n * D;
      CHECK(o1 >= 0 && o1 + one <= o2 && o2 + one <= ws);      // l1, then l2, both inside the reserve, no overlap
    }
  }
  CHECK(penta_ws_doubles((int64_t)1 << 31, 128) == ((int64_t)1 << 39));
  CHECK(penta_slabs(40) == 1 && penta_slabs(64) == 1 && penta_slabs(65) == 2);
}

int main() {
  chains();
  plan();
  if (bad) {
    printf("traj_penta_check: %d failures\n", bad);
    return 1;
  }
  printf("traj_penta_check: ok\n");
  return 0;
}
