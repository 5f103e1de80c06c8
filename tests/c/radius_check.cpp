// radius_check.cpp -- stand-alone driver of the group radius's host code (csrc/gmmmap_prepare.cpp: screen_radius_table,
// screen_radius_lmin, through vcmi_debug_screen_radius) for the ASan + UBSan build of tests/test_screen_radius_host.py: dimensions
// that do and do not fill a k-step, two to sixty-four mixtures, a zero-weight one, prune 0, 46 and +inf.  The values are checked by
// the Python test; here a read or write past a table is the finding.
#include <cstdio>
#include <cmath>
#include <vector>
#include <random>
extern "C" int vcmi_debug_screen_radius(const double *w, const double *mu, const double *sigma, int Dj, int M, int swap, double prune,
                                        double *c, double *R, double *lmin, double *pass_frac);
extern "C" const char *vcmi_last_error(void);
int main() {
  for (int D : {16, 18, 40}) for (int M : {2, 7, 64}) {
    const int Dj = 2 * D;
    std::mt19937_64 rng(D * 100 + M);
    std::normal_distribution<double> nd;
    std::vector<double> w(M, 1.0 / M), mu((size_t)Dj * M), sig((size_t)Dj * Dj * M, 0.0);
    if (M > 2) w[1] = 0.0;
    for (auto &v : mu) v = nd(rng);
    for (int m = 0; m < M; ++m) {
      std::vector<double> B((size_t)Dj * Dj);
      for (auto &v : B) v = 0.05 * nd(rng);
      for (int r = 0; r < Dj; ++r) for (int c = 0; c < Dj; ++c) {
        double s = (r == c) ? 1e-3 : 0.0;
        for (int k = 0; k < Dj; ++k) s += B[(size_t)r * Dj + k] * B[(size_t)c * Dj + k];
        sig[(size_t)Dj * Dj * m + r + (size_t)Dj * c] = s;
      }
    }
    std::vector<double> c((size_t)M * M * 7), R(M), lmin(M);
    double frac = -1;
    for (double prune : {0.0, 46.0, 1e301}) {
      int rc = vcmi_debug_screen_radius(w.data(), mu.data(), sig.data(), Dj, M, 0, prune, c.data(), R.data(), lmin.data(), &frac);
      if (rc) { printf("rc %d %s\n", rc, vcmi_last_error()); return 1; }
    }
    printf("D %d M %d R0 %g lmin0 %g frac %g\n", D, M, R[0], lmin[0], frac);
  }
  printf("radius_check: ok\n");
  return 0;
}
