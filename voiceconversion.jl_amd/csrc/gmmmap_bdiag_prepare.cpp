// gmmmap_bdiag_prepare.cpp -- see gmmmap_bdiag_prepare.hpp.  Host code only.
#include "gmmmap_bdiag_prepare.hpp"
#include "bdiag_pair.hpp"

#include <cmath>
#include <limits>

namespace vcmi {

static constexpr double kLog2Pi = 1.8378770664093454835606594728112;

int64_t bdmap_prepare(const double *weights, const double *mu, const double *covars, int Dj, int M, bool swap, BdmapTable *out) {
  const int D = Dj / 2, DP = (D + 3) & ~3;
  const int64_t bad = first_bad_pair(covars, Dj, M);
  if (bad >= 0) return bad;
  out->D = D;
  out->DP = DP;
  out->M = M;
  out->prm1.assign((size_t)M * DP * kBdmapPrm1, 0.0);
  out->prm3.assign((size_t)M * DP * kBdmapPrm3, 0.0);
  out->cst.assign((size_t)M, 0.0);
  out->a.assign((size_t)M * D, 0.0);
  out->q.assign((size_t)M * D, 0.0);
  out->prm4.assign((size_t)M * DP * kBdmapPrm4, 0.0);
  out->q_bad = -1;
  const int xo = swap ? D : 0, yo = swap ? 0 : D;       // rows of the source and of the target half
  for (int m = 0; m < M; ++m) {
    const double *mm = mu + (size_t)m * Dj, *cv = covars + (size_t)m * (Dj + D);
    double s = 0.0, comp = 0.0;                          // Neumaier: s + comp is the sum of the logarithms to about an ulp
    for (int d = 0; d < D; ++d) {
      const double vx = cv[xo + d], c = cv[Dj + d];
      double *p1 = out->prm1.data() + ((size_t)m * DP + d) * kBdmapPrm1, *p3 = out->prm3.data() + ((size_t)m * DP + d) * kBdmapPrm3;
      p1[0] = p3[0] = mm[xo + d];
      p1[1] = 1.0 / vx;
      p3[1] = c / vx;
      p3[2] = mm[yo + d];
      out->a[(size_t)m * D + d] = p3[1];
      // the conditional variance v_y - a c with one rounding, whatever the compiler contracts elsewhere
      const double cvar = std::fma(-p3[1], c, cv[yo + d]), q = 1.0 / cvar;
      if (!(cvar > 0.0 && std::isfinite(cvar)) && out->q_bad < 0) out->q_bad = d + (int64_t)D * m;
      double *p4 = out->prm4.data() + ((size_t)m * DP + d) * kBdmapPrm4;
      p4[0] = p3[0];
      p4[1] = p3[1];
      p4[2] = p3[2];
      p4[3] = q;
      out->q[(size_t)m * D + d] = q;
      const double lv = std::log(vx), t = s + lv;
      comp += (std::fabs(s) >= std::fabs(lv)) ? (s - t) + lv : (lv - t) + s;
      s = t;
    }
    const double w = weights[m];
    out->cst[m] = (w > 0.0) ? std::log(w) - 0.5 * (D * kLog2Pi + (s + comp)) : -std::numeric_limits<double>::infinity();
  }
  return -1;
}

}  // namespace vcmi
