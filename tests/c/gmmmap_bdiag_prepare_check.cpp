// gmmmap_bdiag_prepare_check.cpp -- stand-alone check of csrc/gmmmap_bdiag_prepare.cpp (no device, no HIP): the table the
// cross-diagonal convert kernel reads against long-double values, the -infinity constant of a mixture without weight, and the
// first-bad-pair report.  Built by tests/test_gmmmap_bdiag_host.py with ASan + UBSan, so a write past a table is a finding too.
#include "../../voiceconversion.jl_amd/csrc/gmmmap_bdiag_prepare.hpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

using namespace vcmi;

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++failures;                        \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
    }                                    \
  } while (0)

struct Model {
  int Dj, M;
  std::vector<double> w, mu, cov;
};

static Model make(int D, int M, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> N(0.0, 1.0);
  Model g{2 * D, M, std::vector<double>(M), std::vector<double>((size_t)2 * D * M), std::vector<double>((size_t)3 * D * M)};
  double s = 0.0;
  for (double &x : g.w) s += (x = 0.1 + U(rng));
  for (double &x : g.w) x /= s;
  for (double &x : g.mu) x = 3.0 * N(rng);
  for (int m = 0; m < M; ++m) {
    double *cv = g.cov.data() + (size_t)m * 3 * D;
    for (int d = 0; d < 2 * D; ++d) cv[d] = std::exp(std::log(1e-7) + U(rng) * std::log(1e9));     // variances in [1e-7, 100]
    for (int d = 0; d < D; ++d) cv[2 * D + d] = (1.8 * U(rng) - 0.9) * std::sqrt(cv[d] * cv[D + d]);
  }
  return g;
}

static double ulps(double got, long double want) {
  const double w = (double)want;
  if (got == w) return 0.0;
  const double u = std::nextafter(std::fabs(w), INFINITY) - std::fabs(w);
  return (double)(std::fabs((long double)got - want) / u);
}

static void check_table(int D, int M, bool swap) {
  Model g = make(D, M, 100u + D + 1000u * M + (swap ? 7u : 0u));
  if (M > 1) g.w[M / 2] = 0.0;                      // a mixture without weight
  BdmapTable t;
  const int64_t bad = bdmap_prepare(g.w.data(), g.mu.data(), g.cov.data(), g.Dj, M, swap, &t);
  CHECK(bad == -1, "D=%d M=%d swap=%d: valid model refused at %lld", D, M, (int)swap, (long long)bad);
  if (bad != -1) return;
  CHECK(t.D == D && t.M == M && t.DP == ((D + 3) & ~3), "dims %d %d %d", t.D, t.DP, t.M);
  CHECK(t.prm1.size() == (size_t)M * t.DP * kBdmapPrm1 && t.prm3.size() == (size_t)M * t.DP * kBdmapPrm3 && t.cst.size() == (size_t)M && t.a.size() == (size_t)M * D, "sizes");
  if (failures) return;
  const long double log2pi = std::log(2.0L * std::acos(-1.0L));
  const int xo = swap ? D : 0, yo = swap ? 0 : D;
  double worst = 0.0;
  for (int m = 0; m < M; ++m) {
    const double *mu = g.mu.data() + (size_t)m * 2 * D, *cv = g.cov.data() + (size_t)m * 3 * D;
    long double sl = 0.0L;
    for (int d = 0; d < D; ++d) {
      const double *p1 = t.prm1.data() + ((size_t)m * t.DP + d) * kBdmapPrm1, *p3 = t.prm3.data() + ((size_t)m * t.DP + d) * kBdmapPrm3;
      const long double vx = cv[xo + d], c = cv[2 * D + d];
      CHECK(p1[0] == mu[xo + d] && p3[0] == mu[xo + d] && p3[2] == mu[yo + d] && p3[3] == 0.0, "means of (%d,%d)", d, m);
      const double e1 = ulps(p1[1], 1.0L / vx), e2 = ulps(p3[1], c / vx);
      CHECK(e1 <= 0.5 && e2 <= 0.5, "1/vx, a of (%d,%d): %g %g ulps", d, m, e1, e2);
      CHECK(t.a[(size_t)m * D + d] == p3[1], "slope copy of (%d,%d)", d, m);
      sl += std::log(vx);
    }
    for (int d = D; d < t.DP; ++d) {
      for (int k = 0; k < kBdmapPrm1; ++k) CHECK(t.prm1[((size_t)m * t.DP + d) * kBdmapPrm1 + k] == 0.0, "padding row");
      for (int k = 0; k < kBdmapPrm3; ++k) CHECK(t.prm3[((size_t)m * t.DP + d) * kBdmapPrm3 + k] == 0.0, "padding row");
    }
    if (!(g.w[m] > 0.0)) {
      CHECK(t.cst[m] == -std::numeric_limits<double>::infinity(), "constant of the weightless mixture %d: %g", m, t.cst[m]);
      continue;
    }
    const long double want = std::log((long double)g.w[m]) - 0.5L * (D * log2pi + sl);
    // every term enters with at most an ulp of itself (the library's log) and the compensated sum adds about one of the total:
    // measured in ulps of the LARGEST magnitude that enters, a few
    long double scale = std::fabs(want);
    scale = std::fmax(scale, std::fabs(0.5L * sl));
    scale = std::fmax(scale, 0.5L * D * log2pi);
    const double u = std::nextafter((double)scale, INFINITY) - (double)scale;
    const double e = (double)(std::fabs((long double)t.cst[m] - want) / u);
    worst = std::fmax(worst, e);
    CHECK(e <= 4.0, "constant of mixture %d (D=%d): %g ulps of %Lg", m, D, e, scale);
  }
  std::printf("D=%3d M=%3d swap=%d: constants within %.2f ulps\n", D, M, (int)swap, worst);
}

static void check_bad_pairs(bool swap) {
  const int D = 5, M = 3;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  struct Case {
    const char *what;
    int d, m, row;      // row 0: vx, 1: vy, 2: c
    double value;
  } cases[] = {{"vx = 0", 2, 1, 0, 0.0},   {"vy = 0", 4, 0, 1, 0.0}, {"vx < 0", 0, 2, 0, -1.0},
               {"NaN variance", 3, 1, 1, nan}, {"NaN c", 1, 2, 2, nan}};
  for (const Case &c : cases) {
    Model g = make(D, M, 5u);
    g.cov[(size_t)c.m * 3 * D + c.row * D + c.d] = c.value;
    BdmapTable t;
    t.D = -7;
    const int64_t bad = bdmap_prepare(g.w.data(), g.mu.data(), g.cov.data(), g.Dj, M, swap, &t);
    CHECK(bad == c.d + (int64_t)D * c.m, "%s swap=%d: reported %lld, expected %d", c.what, (int)swap, (long long)bad, c.d + D * c.m);
    CHECK(t.D == -7 && t.prm1.empty() && t.prm3.empty(), "%s: the table was touched", c.what);
  }
  {   // det < 0: |c| beyond sqrt(vx vy); and det == 0 exactly
    Model g = make(D, M, 6u);
    double *cv = g.cov.data() + (size_t)2 * 3 * D;
    cv[2 * D + 3] = 1.0001 * std::sqrt(cv[3] * cv[D + 3]);
    BdmapTable t;
    CHECK(bdmap_prepare(g.w.data(), g.mu.data(), g.cov.data(), g.Dj, M, swap, &t) == 3 + D * 2, "det < 0 swap=%d", (int)swap);
    cv[2 * D + 3] = 0.0;
    cv[1] = 4.0, cv[D + 1] = 9.0, cv[2 * D + 1] = 6.0;
    CHECK(bdmap_prepare(g.w.data(), g.mu.data(), g.cov.data(), g.Dj, M, swap, &t) == 1 + D * 2, "det == 0 swap=%d", (int)swap);
  }
  {   // two bad pairs: the first in memory order (mixture-major) is named
    Model g = make(D, M, 7u);
    g.cov[(size_t)2 * 3 * D + 0] = -1.0;       // (0, 2)
    g.cov[(size_t)1 * 3 * D + 4] = 0.0;        // (4, 1): earlier in memory
    BdmapTable t;
    CHECK(bdmap_prepare(g.w.data(), g.mu.data(), g.cov.data(), g.Dj, M, swap, &t) == 4 + D * 1, "first of two swap=%d", (int)swap);
  }
}

int main() {
  const int Ds[] = {1, 3, 41, 128}, Ms[] = {1, 17, 256};
  for (int D : Ds)
    for (int M : Ms)
      for (int swap = 0; swap < 2; ++swap) check_table(D, M, swap != 0);
  check_bad_pairs(false);
  check_bad_pairs(true);
  if (failures) {
    std::printf("gmmmap_bdiag_prepare_check: %d failures\n", failures);
    return 1;
  }
  std::printf("gmmmap_bdiag_prepare_check: ok\n");
  return 0;
}
