// traj_bdiag_prepare_check.cpp -- stand-alone check of what csrc/gmmmap_bdiag_prepare.cpp makes for trajectory conversion
// straight from a cross-diagonal model (vcmi_traj_create_bdiag; no device, no HIP): q and the [mu_x, a, mu_y, q] table bit for
// bit against the plain expressions, zero padding rows, the report of a VALID pair whose conditional variance rounds to zero or
// below, and the frame-by-frame tables (prm1, prm3, cst, a) against values computed here: the extension leaves them as they were.
// Built by tests/test_traj_bdiag_host.py with ASan + UBSan, so a write past a table is a finding too.
#include "../../voiceconversion.jl_amd/csrc/bdiag_pair.hpp"
#include "../../voiceconversion.jl_amd/csrc/gmmmap_bdiag_prepare.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Model {
  int Dj, M;
  std::vector<double> w, mu, cov;
};

// Dj: the joint dimension bdmap_prepare takes (4 x the static dimension of a trajectory model); D = Dj / 2 pairs
static Model make(int Dj, int M, unsigned seed) {
  const int D = Dj / 2;
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> N(0.0, 1.0);
  Model g{Dj, M, std::vector<double>(M), std::vector<double>((size_t)Dj * M), std::vector<double>((size_t)3 * D * M)};
  double s = 0.0;
  for (double &x : g.w) s += (x = 0.1 + U(rng));
  for (double &x : g.w) x /= s;
  for (double &x : g.mu) x = 3.0 * N(rng);
  for (int m = 0; m < M; ++m) {
    double *cv = g.cov.data() + (size_t)m * 3 * D;
    for (int d = 0; d < Dj; ++d) cv[d] = std::exp(std::log(1e-7) + U(rng) * std::log(1e9));     // variances in [1e-7, 100]
    for (int d = 0; d < D; ++d) cv[Dj + d] = (1.8 * U(rng) - 0.9) * std::sqrt(cv[d] * cv[D + d]);
  }
  return g;
}

static void check_tables(int Dj, int M, bool swap) {
  const int D = Dj / 2, DP = (D + 3) & ~3;
  Model g = make(Dj, M, 300u + Dj + 1000u * M + (swap ? 7u : 0u));
  if (M > 1) g.w[M / 2] = 0.0;                      // a mixture without weight: its q and its rows are made all the same
  BdmapTable t;
  const int64_t bad = bdmap_prepare(g.w.data(), g.mu.data(), g.cov.data(), Dj, M, swap, &t);
  CHECK(bad == -1, "Dj=%d M=%d swap=%d: valid model refused at %lld", Dj, M, (int)swap, (long long)bad);
  if (bad != -1) return;
  CHECK(t.D == D && t.M == M && t.DP == DP, "dims %d %d %d", t.D, t.DP, t.M);
  CHECK(t.q.size() == (size_t)M * D && t.prm4.size() == (size_t)M * DP * kBdmapPrm4, "sizes of q and the trajectory table");
  CHECK(t.prm1.size() == (size_t)M * DP * kBdmapPrm1 && t.prm3.size() == (size_t)M * DP * kBdmapPrm3 && t.cst.size() == (size_t)M &&
            t.a.size() == (size_t)M * D, "sizes of the frame-by-frame tables");
  CHECK(t.q_bad == -1, "Dj=%d M=%d swap=%d: q_bad %lld on a model with correlations below 0.9", Dj, M, (int)swap, (long long)t.q_bad);
  if (failures) return;
  const int xo = swap ? D : 0, yo = swap ? 0 : D;
  const double log2pi = 1.8378770664093454835606594728112;
  for (int m = 0; m < M; ++m) {
    const double *mu = g.mu.data() + (size_t)m * Dj, *cv = g.cov.data() + (size_t)m * 3 * D;
    double s = 0.0, comp = 0.0;
    for (int d = 0; d < D; ++d) {
      const double vx = cv[xo + d], vy = cv[yo + d], c = cv[Dj + d];
      const double a = c / vx, q = 1.0 / std::fma(-a, c, vy);          // the plain expressions (the one fma is the statement's)
      const double *p1 = t.prm1.data() + ((size_t)m * DP + d) * kBdmapPrm1, *p3 = t.prm3.data() + ((size_t)m * DP + d) * kBdmapPrm3,
                   *p4 = t.prm4.data() + ((size_t)m * DP + d) * kBdmapPrm4;
      CHECK(same_bits(t.q[(size_t)m * D + d], q) && q > 0.0, "q of (%d,%d): %a, expected %a", d, m, t.q[(size_t)m * D + d], q);
      CHECK(same_bits(p4[0], mu[xo + d]) && same_bits(p4[1], a) && same_bits(p4[2], mu[yo + d]) && same_bits(p4[3], q),
            "trajectory row of (%d,%d)", d, m);
      // the frame-by-frame tables, as before the extension
      CHECK(same_bits(p1[0], mu[xo + d]) && same_bits(p1[1], 1.0 / vx), "prm1 of (%d,%d)", d, m);
      CHECK(same_bits(p3[0], mu[xo + d]) && same_bits(p3[1], a) && same_bits(p3[2], mu[yo + d]) && same_bits(p3[3], 0.0),
            "prm3 of (%d,%d)", d, m);
      CHECK(same_bits(t.a[(size_t)m * D + d], a), "slope copy of (%d,%d)", d, m);
      const double lv = std::log(vx), u = s + lv;                     // the Neumaier sum of the header's statement
      comp += (std::fabs(s) >= std::fabs(lv)) ? (s - u) + lv : (lv - u) + s;
      s = u;
    }
    for (int d = D; d < DP; ++d)
      for (int k = 0; k < 4; ++k) {
        CHECK(same_bits(t.prm4[((size_t)m * DP + d) * kBdmapPrm4 + k], 0.0), "padding row %d of the trajectory table", d);
        CHECK(same_bits(t.prm3[((size_t)m * DP + d) * kBdmapPrm3 + k], 0.0), "padding row %d of prm3", d);
        if (k < kBdmapPrm1) CHECK(same_bits(t.prm1[((size_t)m * DP + d) * kBdmapPrm1 + k], 0.0), "padding row %d of prm1", d);
      }
    const double want = (g.w[m] > 0.0) ? std::log(g.w[m]) - 0.5 * (D * log2pi + (s + comp)) : -std::numeric_limits<double>::infinity();
    CHECK(same_bits(t.cst[m], want), "constant of mixture %d: %a, expected %a", m, t.cst[m], want);
  }
  std::printf("Dj=%3d M=%d swap=%d: q, the trajectory table and the frame-by-frame tables bit for bit\n", Dj, M, (int)swap);
}

// A pair that IS positive definite (Kahan's determinant > 0) and whose conditional variance fma(-fl(c / vx), c, vy) is negative:
// |c| a few ulps below sqrt(vx vy), a = c / vx rounded up.  bdmap_prepare accepts the model (the frame-by-frame converter needs
// v_x alone) and names the pair in q_bad: VCMI_ERR_NOT_PD at trajectory creation.
static void check_not_pd() {
  const int Dj = 12, D = 6, M = 3;
  const struct {
    double vx, vy, c;
  } pairs[] = {{0x1.40c25bc0b494dp+1, 0x1.ce0f24a25593fp-1, 0x1.80faec4f29850p+0},
               {0x1.806f1224208aap+1, 0x1.c4d2afc20511dp+1, 0x1.a13ac3b5eda68p+1},
               {0x1.9e8c8144740bcp+0, 0x1.17b0f61c86433p+1, 0x1.e18d0efbb4235p+0}};
  for (const auto &p : pairs) {
    CHECK(bdiag_pair_valid(p.vx, p.vy, p.c), "the pair of the case is valid");
    CHECK(!(std::fma(-(p.c / p.vx), p.c, p.vy) > 0.0), "its conditional variance rounds to zero or below");
  }
  for (int swap = 0; swap < 2; ++swap) {
    {   // one such pair at (4, 1)
      Model g = make(Dj, M, 11u);
      double *cv = g.cov.data() + (size_t)1 * 3 * D;
      cv[(swap ? D : 0) + 4] = pairs[0].vx, cv[(swap ? 0 : D) + 4] = pairs[0].vy, cv[Dj + 4] = pairs[0].c;
      BdmapTable t;
      CHECK(bdmap_prepare(g.w.data(), g.mu.data(), g.cov.data(), Dj, M, swap != 0, &t) == -1, "the model converts frame by frame");
      CHECK(t.q_bad == 4 + (int64_t)D * 1, "swap=%d: q_bad %lld, expected %d", swap, (long long)t.q_bad, 4 + D * 1);
      CHECK(!(t.q[(size_t)1 * D + 4] > 0.0) || std::isinf(t.q[(size_t)1 * D + 4]), "the entry holds what the division gave");
    }
    {   // two: the first in memory order (mixture-major) is named
      Model g = make(Dj, M, 12u);
      double *c2 = g.cov.data() + (size_t)2 * 3 * D, *c0 = g.cov.data();
      c2[(swap ? D : 0) + 0] = pairs[1].vx, c2[(swap ? 0 : D) + 0] = pairs[1].vy, c2[Dj + 0] = pairs[1].c;     // (0, 2)
      c0[(swap ? D : 0) + 5] = pairs[2].vx, c0[(swap ? 0 : D) + 5] = pairs[2].vy, c0[Dj + 5] = pairs[2].c;     // (5, 0): earlier
      BdmapTable t;
      CHECK(bdmap_prepare(g.w.data(), g.mu.data(), g.cov.data(), Dj, M, swap != 0, &t) == -1, "the model converts frame by frame");
      CHECK(t.q_bad == 5, "swap=%d: first of two: q_bad %lld", swap, (long long)t.q_bad);
    }
  }
  {   // an invalid pair is still refused outright, the table untouched
    Model g = make(Dj, M, 13u);
    g.cov[(size_t)1 * 3 * D + 2] = 0.0;
    BdmapTable t;
    t.q_bad = -5;
    CHECK(bdmap_prepare(g.w.data(), g.mu.data(), g.cov.data(), Dj, M, false, &t) == 2 + D * 1, "vx = 0 is the pair's own refusal");
    CHECK(t.q_bad == -5 && t.q.empty() && t.prm4.empty(), "the table was touched");
  }
}

int main() {
  const int shapes[][2] = {{4, 1}, {12, 3}, {256, 2}};
  for (const auto &s : shapes)
    for (int swap = 0; swap < 2; ++swap) check_tables(s[0], s[1], swap != 0);
  check_not_pd();
  if (failures) {
    std::printf("traj_bdiag_prepare_check: %d failures\n", failures);
    return 1;
  }
  std::printf("traj_bdiag_prepare_check: ok\n");
  return 0;
}
