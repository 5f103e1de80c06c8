// gmmmap_prepare.cpp -- host-side preparation of a GMMMap converter: the joint GMM becomes the device images that the
// kernels of gmmmap.hip read.  Host code only (no kernel lives here, so an edit does not recompile one).
//
// Replaces:
//   GMMMap ctor / GMMMapParam / split_joint_gmm          reference src/gmmmap.jl:23-90
//   GaussianMixtureModel (Hermitian + Cholesky)          reference src/gmm.jl:8-20
//
// Math.  Per mixture m:
//   A_m = Syx_m inv(Sxx_m)              b_m  = muy_m - A_m mux_m
//   L_m L_m' = Hermitian(Sxx_m)         U_m  = inv(L_m)   (lower triangular)     cz_m = U_m mux_m
//   lc_m = log w_m - (D log 2pi + 2 sum_i log L_m[i,i]) / 2
// gmmmap_prepare() at the end of the file is the sequence: factor_model, profile_model, choose_screen_rows, then one packer
// and one upload per image.  The layouts the packers write are those of gmmmap_layout.hpp.
#include "gmmmap_prepare.hpp"
#include "bf16_split.hpp"
#include "host_linalg.hpp"
#include "hostpipe.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>

namespace vcmi {

// ------------------------------------------------------------------------------------------------
// factorisation
// ------------------------------------------------------------------------------------------------
int factor_model(vcmi_gmmmap *g, HostModel &hm, const double *w, const double *mu, const double *sigma, int Dj, int M, int swap,
                 bool px_only) {
  const int D = px_only ? Dj : Dj >> 1;   // src/gmmmap.jl:70
  const int DP = (D + 3) / 4 * 4;
  const size_t dd = (size_t)D * D, pp = (size_t)DP * DP;
  const size_t reg = px_only ? 0 : 1;   // the regression side (A, b, Sxy, Syy) does not exist for a p(x)-only handle
  for (std::vector<double> *h : {&g->h_A_julia, &g->h_Sxy, &g->h_Syy, &g->h_A}) h->assign(reg * dd * M, 0.0);
  for (std::vector<double> *h : {&g->h_mux, &g->h_muy}) h->assign((size_t)D * M, 0.0);
  const bool want_screen = !px_only && D >= 4 && gmmmap_has_mfma(DP) && M <= 1024;       // (fvconvert's screen: DP <= 48; predict's: every tile-kernel dimension)
  const bool want_screen2 = want_screen && screen16_has(DP);      // sixteen rows: only where the bf16 screen (and its second look) exists
  using V = std::vector<double>;
  hm = HostModel{D, DP, M, px_only, /*U, A*/ V(pp * M), V(reg * pp * M), /*cz, b*/ V((size_t)DP * M), V(reg * DP * M), /*lc*/ V(M),
                 /*P, cP*/ V(want_screen ? (size_t)M * 4 * DP : 0), V(want_screen ? (size_t)M * 4 : 0),
                 /*P2, cP2*/ V(want_screen2 ? (size_t)M * 16 * DP : 0), V(want_screen2 ? (size_t)M * 16 : 0)};
  // (the group radius of that screen: the Hermitian source blocks themselves, where the M^2 table stays small)
  if (want_screen && screen_has_kernel(DP) && M >= 2 && M <= ScreenRadius::kMaxM) hm.Sxx.assign(dd * M, 0.0);
  V &hU = hm.U, &hA = hm.A, &hcz = hm.cz, &hb = hm.b, &hlc = hm.lc, &hP = hm.P, &hcP = hm.cP, &hP2 = hm.P2, &hcP2 = hm.cP2;
  const int xo = (swap && !px_only) ? D : 0, yo = px_only ? 0 : (swap ? 0 : D);   // src/gmmmap.jl:74-78
  const double LOG2PI = 1.8378770664093454835606594728112;
  // The mixtures are independent (an inverse, a Cholesky factorisation and a triangular inverse each: 64 x 160^3 flop for
  // the joint model of delta features): they are shared out over the library's host threads.  The first failing mixture
  // (lowest index) is reported, as the sequential loop would.
  std::atomic<int> bad_singular{M}, bad_notpd{M};
  auto lower_to = [](std::atomic<int> &a, int v) {
    int cur = a.load();
    while (v < cur && !a.compare_exchange_weak(cur, v)) {}
  };
  host_parallel_for(M, 1, [&](int64_t m_lo, int64_t m_hi) {
  std::vector<double> Sxx(dd), Syx(dd), inv(dd), L(dd), Ui(dd);
  for (int m = (int)m_lo; m < (int)m_hi; ++m) {
    const double *S = sigma + (size_t)Dj * Dj * m;   // column-major (Dj,Dj)
    double *mux = &g->h_mux[(size_t)D * m], *muy = &g->h_muy[(size_t)D * m];
    for (int d = 0; d < D; ++d) {
      mux[d] = mu[xo + d + (size_t)Dj * m];
      muy[d] = px_only ? 0.0 : mu[yo + d + (size_t)Dj * m];
    }
    // row-major copies of the four blocks, src/gmmmap.jl:41-52
    for (int r = 0; r < D; ++r)
      for (int c = 0; c < D; ++c) {
        Sxx[(size_t)r * D + c] = S[(xo + r) + (size_t)Dj * (xo + c)];
        if (px_only) continue;
        Syx[(size_t)r * D + c] = S[(yo + r) + (size_t)Dj * (xo + c)];
        g->h_Sxy[dd * m + (size_t)r * D + c] = S[(xo + r) + (size_t)Dj * (yo + c)];
        g->h_Syy[dd * m + (size_t)r * D + c] = S[(yo + r) + (size_t)Dj * (yo + c)];
      }
    // A_m = Syx inv(Sxx) on the raw block, src/gmmmap.jl:35
    double *Am = px_only ? nullptr : &g->h_A[dd * m];
    if (!px_only) {
      if (!la::inverse(Sxx.data(), D, inv.data())) {
        lower_to(bad_singular, m);
        continue;
      }
      la::matmul(Syx.data(), inv.data(), D, Am);
      for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
          g->h_A_julia[dd * m + r + (size_t)D * c] = Am[(size_t)r * D + c];
          hA[pp * m + (size_t)r * DP + c] = Am[(size_t)r * D + c];
        }
    }
    // p(x): Hermitian(Sxx) (upper triangle mirrored, src/gmm.jl:16) -> Cholesky -> U = inv(L)
    if (!la::cholesky_from_upper(Sxx.data(), D, L.data())) {
      lower_to(bad_notpd, m);
      continue;
    }
    la::lower_inverse(L.data(), D, Ui.data());
    if (!hm.Sxx.empty())
      for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) hm.Sxx[dd * m + (size_t)r * D + c] = r <= c ? Sxx[(size_t)r * D + c] : Sxx[(size_t)c * D + r];
    double logdiag = 0.0;
    for (int d = 0; d < D; ++d) logdiag += std::log(L[(size_t)d * D + d]);
    hlc[m] = (w[m] > 0.0) ? std::log(w[m]) - 0.5 * (D * LOG2PI + 2.0 * logdiag)
                          : -std::numeric_limits<double>::infinity();   // zero-weight: posterior 0
    for (int r = 0; r < D; ++r) {
      double cz = 0.0, ba = 0.0;
      for (int c = 0; c < D; ++c) {
        hU[pp * m + (size_t)r * DP + c] = Ui[(size_t)r * D + c];
        cz += Ui[(size_t)r * D + c] * mux[c];
        if (!px_only) ba += Am[(size_t)r * D + c] * mux[c];
      }
      hcz[(size_t)DP * m + r] = cz;
      if (!px_only) hb[(size_t)DP * m + r] = muy[r] - ba;
    }
    // screening rows of shape 3 (gmmmap_screen.hpp): P_m = diag(sqrt(kappa_i)) v_i' over the FOUR LARGEST eigenpairs of
    // inv(Sxx_m) = U'U -- the directions of smallest variance.  |P_m (x - mu_m)|^2 is a partial sum of the eigen-expansion of
    // (x - mu_m)' inv(Sxx_m) (x - mu_m) = |z_m|^2: a lower bound of it, and per row the largest one any direction can give.
    if (want_screen) {
      std::vector<double> G(dd), V(dd);
      for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
          double sacc = 0.0;
          for (int k = std::max(r, c); k < D; ++k) sacc += Ui[(size_t)k * D + r] * Ui[(size_t)k * D + c];
          G[(size_t)r * D + c] = sacc;
        }
      la::sym_eigen_jacobi(G.data(), D, V.data());
      // (where the bf16 screen exists the sixteen strongest go to P2 for its second look; the first four are P)
      const int nrows = want_screen2 ? std::min(16, D) : 4;
      int top[16];
      for (int i = 0; i < nrows; ++i) {
        double bestv = -1.0;
        top[i] = -1;
        for (int j = 0; j < D; ++j) {
          bool used = false;
          for (int u = 0; u < i; ++u) used = used || top[u] == j;
          if (!used && G[(size_t)j * D + j] > bestv) {
            bestv = G[(size_t)j * D + j];
            top[i] = j;
          }
        }
        const double sk = std::sqrt(std::max(bestv, 0.0));
        double cp = 0.0;
        for (int k = 0; k < D; ++k) {
          const double v = sk * V[(size_t)k * D + top[i]];
          if (want_screen2) hP2[((size_t)m * 16 + i) * DP + k] = v;
          if (i < 4) hP[((size_t)m * 4 + i) * DP + k] = v;
          cp += v * mux[k];
        }
        if (want_screen2) hcP2[(size_t)m * 16 + i] = cp;
        if (i < 4) hcP[(size_t)m * 4 + i] = cp;
      }
    }
  }
  });
  {
    const int bs = bad_singular.load(), bp = bad_notpd.load();
    if (bs < M && bs <= bp) return fail(VCMI_ERR_NOT_PD, "Sigma^xx of mixture %d is singular", bs + 1);
    if (bp < M) return fail(VCMI_ERR_NOT_PD, "Sigma^xx of mixture %d is not positive definite", bp + 1);
  }
  return VCMI_OK;
}

// ------------------------------------------------------------------------------------------------
// profile
// ------------------------------------------------------------------------------------------------
// How broad is the model?  256 frames are drawn from p(x) itself (stratified over the weights, fixed-seed normal deviates:
// x = mu_m + L_m z, i.e. U_m (x - mu_m) = z solved by forward substitution) and for each the mixtures within e^-46 of the best
// one are counted -- in full, on the last whitening tile's share alone, and on the screening rows alone.  The means over the
// frames, as fractions of the M mixtures.  A property of the model only; it selects the loop SHAPE of fvconvert
// (convert_shape, gmmmap.hip), never a result.
ModelProfile profile_model(const HostModel &hm, const std::vector<double> &hmux, const double *w) {
  const std::vector<double> &hU = hm.U, &hcz = hm.cz, &hlc = hm.lc, &hP = hm.P, &hcP = hm.cP;
  const int D = hm.D, DP = hm.DP, M = hm.M;
  ModelProfile pf;
  constexpr int S = 256;
  const size_t pp = (size_t)DP * DP;
  std::vector<double> cdf(M);
  double tot = 0.0;
  for (int m = 0; m < M; ++m) cdf[m] = (tot += (w[m] > 0.0 ? w[m] : 0.0));
  if (!(tot > 0.0) || M < 2) return pf;
  // per frame, the mixtures {within e^-46 of the best | ... on the last 16-row whitening tile's share alone | whose bound from
  // four rows reaches the best log-density (predict's screen) | ... on the 4 / 2 / 1 strongest screening rows alone (shape 3)}
  std::vector<int> tally(6 * S, 0);
  pf.own_m.assign(S, 0);
  pf.own_z2.assign(S, 0.0);
  const int r_last = 16 * ((DP + 15) / 16 - 1);                       // first row of the last whitening tile
  host_parallel_for(S, 8, [&](int64_t lo, int64_t hi) {
    std::vector<double> x(D), z(D);
    for (int s = (int)lo; s < (int)hi; ++s) {
      const double u = (s + 0.5) / S * tot;
      int m = 0;
      while (m + 1 < M && cdf[m] < u) ++m;
      uint64_t st = 0x9E3779B97F4A7C15ull * (uint64_t)(s + 1);          // splitmix64 stream per frame
      auto rnd = [&]() {
        st += 0x9E3779B97F4A7C15ull;
        uint64_t v = st;
        v = (v ^ (v >> 30)) * 0xBF58476D1CE4E5B9ull;
        v = (v ^ (v >> 27)) * 0x94D049BB133111EBull;
        v ^= v >> 31;
        return ((double)(v >> 11) + 0.5) * (1.0 / 9007199254740992.0);
      };
      for (int d = 0; d < D; d += 2) {                                  // Box-Muller
        const double r = std::sqrt(-2.0 * std::log(rnd())), a = 6.283185307179586 * rnd();
        z[d] = r * std::cos(a);
        if (d + 1 < D) z[d + 1] = r * std::sin(a);
      }
      const double *Um = &hU[pp * m];
      for (int r = 0; r < D; ++r) {                                     // U_m (x - mu_m) = z, U_m lower triangular
        double acc = z[r];
        for (int c = 0; c < r; ++c) acc -= Um[(size_t)r * DP + c] * x[c];
        x[r] = acc / Um[(size_t)r * DP + r];
      }
      for (int d = 0; d < D; ++d) x[d] += hmux[(size_t)D * m + d];
      double best = -INFINITY;
      std::vector<double> l(M), qlast(M), qlast4(3 * (size_t)M);
      for (int n = 0; n < M; ++n) {
        const double *Un = &hU[pp * n];
        double q = 0.0, ql = 0.0, ql4[3] = {0.0, 0.0, 0.0};
        for (int r = 0; r < D; ++r) {
          double zz = -hcz[(size_t)DP * n + r];
          for (int c = 0; c <= r; ++c) zz += Un[(size_t)r * DP + c] * x[c];
          q += zz * zz;
          if (r >= r_last) ql += zz * zz;
        }
        if (!hP.empty())
          for (int i = 0; i < 4; ++i) {                                  // the screen's rows: strongest first
            double pz = -hcP[(size_t)n * 4 + i];
            for (int c = 0; c < D; ++c) pz += hP[((size_t)n * 4 + i) * DP + c] * x[c];
            for (int c = 0; c < 3; ++c)
              if (i < (4 >> c)) ql4[c] += pz * pz;
          }
        l[n] = hlc[n] - 0.5 * q;
        if (n == m) {
          pf.own_m[s] = m;
          pf.own_z2[s] = q;
        }
        qlast[n] = ql;
        for (int c = 0; c < 3; ++c) qlast4[3 * (size_t)n + c] = ql4[c];
        best = std::max(best, l[n]);
      }
      int *ty = &tally[6 * s];
      for (int n = 0; n < M; ++n) {
        ty[0] += (l[n] > best - 46.0);
        ty[1] += (hlc[n] - 0.5 * qlast[n] > best - 46.0);
        ty[2] += (hlc[n] - 0.5 * qlast4[3 * (size_t)n] >= best);
        for (int c = 0; c < 3; ++c) ty[3 + c] += (hlc[n] - 0.5 * qlast4[3 * (size_t)n + c] > best - 46.0);
      }
    }
  });
  double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < S; ++s)
    for (int i = 0; i < 6; ++i) sum[i] += tally[6 * s + i];
  pf.active = sum[0] / ((double)S * M);
  pf.undecided = sum[1] / ((double)S * M);
  if (!hP.empty()) pf.argmax_survivors = sum[2] / ((double)S * M);
  for (int c = 0; c < 3; ++c) pf.undecided_rows[c] = sum[3 + c] / ((double)S * M);
  return pf;
}

// rpm = the row count with the smallest estimated cost per 16-frame tile -- KS MFMAs screen 16 / rpm mixtures; a mixture the
// screen does not rule out costs its whole whitening (and usually its regression) for the four waves that share it
int choose_screen_rows(const ModelProfile &pf, int DP, int M) {
  const int KSQ = DP / 4;
  int best = 4;
  double best_cost = 1e300;
  for (int c = 0; c < 3; ++c) {
    const int rpm = 4 >> c;
    const double extra = std::max(0.0, pf.undecided_rows[c] - 1.0 / M);      // wrong mixtures let through, per frame
    const double cost = (double)KSQ * M * rpm / 16.0 + 4.0 * extra * M * (2 * KSQ + 2);
    if (cost < best_cost) {
      best_cost = cost;
      best = rpm;
    }
  }
  return best;
}

// ------------------------------------------------------------------------------------------------
// the group radius of shape 3 (ScreenRadius, gmmmap_handle.hpp)
// ------------------------------------------------------------------------------------------------
static double sum_of_squares(const double *v, int n);

ScreenRadius screen_radius_table(const HostModel &hm, const std::vector<double> &hmux) {
  constexpr int J = ScreenRadius::J;
  const int D = hm.D, DP = hm.DP, M = hm.M;
  const size_t dd = (size_t)D * D, pp = (size_t)DP * DP;
  ScreenRadius rt;
  rt.D = D;
  rt.M = M;
  rt.c.assign((size_t)M * M * J, std::numeric_limits<double>::quiet_NaN());
  rt.lc = hm.lc;
  rt.mu_norm.resize(M);
  rt.l_norm.resize(M);
  for (int m = 0; m < M; ++m) {
    rt.mu_norm[m] = std::sqrt(sum_of_squares(&hmux[(size_t)D * m], D));
    double tr = 0.0;                                            // |L_m|_F^2 = trace(Sxx_m)
    for (int d = 0; d < D; ++d) tr += hm.Sxx[dd * m + (size_t)d * D + d];
    rt.l_norm[m] = std::sqrt(tr);
    rt.u_norm = std::max(rt.u_norm, std::sqrt(sum_of_squares(&hm.U[pp * m], (int)pp)));
  }
  // unordered pairs g < m, a row of the triangle per index: the rows are shared out in pairs (g, M - 2 - g) of equal length
  host_parallel_for(M - 1, 1, [&](int64_t lo, int64_t hi) {
    std::vector<double> K(dd), L(dd), d(D), y(D);
    for (int64_t i = lo; i < hi; ++i) {
      const int g = (i & 1) ? M - 2 - (int)(i >> 1) : (int)(i >> 1);
      for (int m = g + 1; m < M; ++m) {
        if (!(hm.lc[g] > -INFINITY) || !(hm.lc[m] > -INFINITY)) continue;      // (a zero-weight mixture is neither a group nor a competitor)
        for (int k = 0; k < D; ++k) d[k] = hmux[(size_t)D * m + k] - hmux[(size_t)D * g + k];
        for (int j = 0; j < J; ++j) {
          const double lam = ScreenRadius::lambda(j), il = 1.0 / lam;
          for (int r = 0; r < D; ++r)
            for (int c = r; c < D; ++c) K[(size_t)r * D + c] = hm.Sxx[dd * m + (size_t)r * D + c] + il * hm.Sxx[dd * g + (size_t)r * D + c];
          if (!la::cholesky_from_upper(K.data(), D, L.data())) continue;
          double q = 0.0;                                       // |inv(L) d|^2 = d' inv(K) d
          for (int r = 0; r < D; ++r) {
            double acc = d[r];
            for (int c = 0; c < r; ++c) acc -= L[(size_t)r * D + c] * y[c];
            y[r] = acc / L[(size_t)r * D + r];
            q += y[r] * y[r];
          }
          rt.c[((size_t)g * M + m) * J + j] = q;
          rt.c[((size_t)m * M + g) * J + (J - 1 - j)] = q * il; // c_mg(1 / lambda) = c_gm(lambda) / lambda
        }
      }
    }
  });
  return rt;
}

// The rounding margin.  The kernel compares FP64 values of l_m = lc_m - |U_m x - cz_m|^2 / 2; the certificate is about the exact
// ones.  For x inside the radius |x| <= X = |mu_g| + sqrt(R) |L_g|_F, so every component sum of U_m x - cz_m (D + 1 terms, each
// at most |U_m row| X) is off by at most (D + 3) eps |U_m row| X and the vector z_m by delta = (D + 3) eps |U_m|_F X in norm --
// whatever the size of x, which is where models shifted by thousands come in.  |z|^2 is then off by 2 |z| delta + delta^2 plus
// (D + 2) eps |z|^2 of its own sum, l by half of that plus eps (|lc| + |z|^2 / 2).  The inequality that has to survive is
// |z_m|^2 - |z_g|^2 - 2 (lc_m - lc_g + prune) > 0 with |z_g|^2 < R and |z_m|^2 >= the bound B <= C = max c: beyond B the left
// side grows faster than its error (1 against delta / |z_m|), so the error at |z_m|^2 = B counts:
//   E = 2 (sqrt(C) + sqrt(R)) delta + 2 delta^2 + 2^-40 (C + R + 4 max |lc| + 2 prune)
// with delta taken sixteen times larger than derived.  R loses FOUR times E (1 + lambda >= 1 turns a loss of R into at least that
// much room in the inequality) and a factor 1 - 2^-20 on top: the benchmark's radii leave 70 nats unused, nothing here is tight.
void screen_radius_lmin(const ScreenRadius &rt, double prune, std::vector<double> &R, std::vector<double> &lmin) {
  constexpr int J = ScreenRadius::J;
  const int M = rt.M;
  R.assign(M, -INFINITY);
  lmin.assign(M, INFINITY);
  double lcmax = 0.0;
  for (int m = 0; m < M; ++m)
    if (rt.lc[m] > -INFINITY) lcmax = std::max(lcmax, std::fabs(rt.lc[m]));
  for (int g = 0; g < M; ++g) {
    if (!(rt.lc[g] > -INFINITY) || !(prune < 1e300)) continue;   // a zero-weight group, the dense loop: nothing is certified
    double r0 = 1e12, cmax = 0.0;                                // (no competitor at all: a radius that still lets a NaN fail)
    for (int m = 0; m < M; ++m) {
      if (m == g || !(rt.lc[m] > -INFINITY)) continue;           // a zero-weight mixture is nobody's competitor
      double best = -INFINITY;
      for (int j = 0; j < J; ++j) {
        const double c = rt.c[((size_t)g * M + m) * J + j];
        if (!(c == c)) continue;
        cmax = std::max(cmax, c);
        best = std::max(best, (c - 2.0 * (rt.lc[m] - rt.lc[g] + prune)) / (1.0 + ScreenRadius::lambda(j)));
      }
      r0 = std::min(r0, best);
    }
    if (!(r0 > 0.0)) continue;
    const double eps = 0x1p-53;
    const double xmax = rt.mu_norm[g] + std::sqrt(r0) * rt.l_norm[g];
    const double delta = 16.0 * (rt.D + 3) * eps * rt.u_norm * xmax;
    const double E = 2.0 * (std::sqrt(cmax) + std::sqrt(r0)) * delta + 2.0 * delta * delta + 0x1p-40 * (cmax + r0 + 4.0 * lcmax + 2.0 * prune);
    const double r = (r0 - 4.0 * E) * (1.0 - 0x1p-20);
    R[g] = r;
    if (r > 0.0) lmin[g] = rt.lc[g] - 0.5 * r;
  }
}

double screen_radius_pass_frac(const ModelProfile &pf, const ScreenRadius &rt, const std::vector<double> &lmin) {
  if (pf.own_m.empty() || rt.empty()) return 0.0;
  int pass = 0;
  for (size_t s = 0; s < pf.own_m.size(); ++s) pass += (rt.lc[pf.own_m[s]] - 0.5 * pf.own_z2[s] >= lmin[pf.own_m[s]]);
  return (double)pass / (double)pf.own_m.size();
}

// The test is taken per WORKGROUP: one frame outside its radius and the 128 of them run the screen after all, one L2 round trip
// later than they would have (stage 0 is then fetched behind the test, not at the top of the kernel).  With a share p of frames
// inside, p^128 of the workgroups skip about a fifth of the kernel and the others lose about a thirtieth of it: even near
// p^128 = 0.15, p = 0.985.  254 of the profile's 256 frames (0.992, p^128 = 0.37) is the first count above that; the peaked
// synthetic models pass with all 256, a model with lam_lo = 1e-2 with a third of them.
bool choose_screen_radius(double pass_frac) { return pass_frac >= 254.0 / 256.0; }

int screen_radius_upload(vcmi_gmmmap *g) {
  if (g->radius.empty()) return VCMI_OK;
  std::vector<double> R, lmin;
  screen_radius_lmin(g->radius, g->prune, R, lmin);
  if (g->grp_order.last_use) VCMI_HIP(hipEventSynchronize(g->grp_order.last_use));      // the last grouped call may still read lmin
  return upload_now(g->lmin, lmin);
}

// ------------------------------------------------------------------------------------------------
// packers: host images -> device images (copies, apart from the norms and margins of the bf16 operands)
// ------------------------------------------------------------------------------------------------
static double sum_of_squares(const double *v, int n) {
  double s = 0.0;
  for (int k = 0; k < n; ++k) s += v[k] * v[k];
  return s;
}

// packed operand blocks for the MFMA kernel, [M][TilingRT::BLK], fragments in issue order (for_each_fragment's variants;
// variant 0 needs the regression side)
std::vector<double> pack_tiles(const HostModel &hm, int variant) {
  const std::vector<double> &hU = hm.U, &hA = hm.A, &hcz = hm.cz, &hb = hm.b, &hlc = hm.lc;
  const int DP = hm.DP, M = hm.M;
  const size_t pp = (size_t)DP * DP;
  const bool uonly = variant != 0;
  const TilingRT tl(DP, uonly);
  std::vector<double> pk((size_t)tl.BLK * M, 0.0);
  auto wrow = [&](int m, int p, int k) -> double {   // row p of [U_m ; A_m], column k
    if (k >= DP) return 0.0;
    if (p < DP) return hU[pp * m + (size_t)p * DP + k];
    if (p < 2 * DP && !uonly) return hA[pp * m + (size_t)(p - DP) * DP + k];
    return 0.0;
  };
  for (int m = 0; m < M; ++m) {
    double *blk = &pk[(size_t)tl.BLK * m];
    int s = 0;
    for_each_fragment(tl, variant, [&](int t, int ks) {
      fill_fragment(blk + (size_t)s * 64, ks, [&](int row, int k) { return wrow(m, 16 * t + row, k); });
      ++s;
    });
    for (int p = 0; p < tl.NT * 16; ++p)
      blk[tl.CINIT_OFF + p] = (p < DP) ? -hcz[(size_t)DP * m + p] : (p < 2 * DP && !uonly) ? hb[(size_t)DP * m + (p - DP)] : 0.0;
    blk[tl.LC_OFF] = hlc[m];
  }
  return pk;
}

// stages of the screen of shape 3 (gmmmap_screen.hpp) on the first rpm rows of every mixture's P_m.  rpm = 4 is also
// predict's screen (gmmmap_screen_argmax_kernel): tile row i <-> mixture i & 3, screening row i >> 2.
std::vector<double> pack_screen(const HostModel &hm, int rpm) {
  const std::vector<double> &hlc = hm.lc, &hP = hm.P, &hcP = hm.cP;
  const int DP = hm.DP, M = hm.M;
  const int KSQ = DP / 4, QFR = screen_frag_doubles(DP), STG = screen_stage_doubles(DP), NQ = screen_quads(DP);
  const int mpt = 16 / rpm, nst = screen_stage_count(DP, M, rpm);
  std::vector<double> pq((size_t)nst * STG, 0.0);
  for (int st = 0; st < nst; ++st)
    for (int q = 0; q < NQ; ++q) {
      const int m0 = (NQ * st + q) * mpt;
      double *fr = &pq[(size_t)st * STG + (size_t)q * KSQ * 64], *cl = &pq[(size_t)st * STG + QFR + (size_t)q * 32];
      for (int ks = 0; ks < KSQ; ++ks)
        fill_fragment(fr + (size_t)ks * 64, ks, [&](int i, int k) {
          const int m = m0 + screen_row_mixture(i, rpm), row = screen_row_index(i, rpm);
          return (m < M && k < DP) ? hP[((size_t)m * 4 + row) * DP + k] : 0.0;
        });
      for (int j = 0; j < 4; ++j) {
        for (int r = 0; r < 4; ++r) {                        // register r of lane group j holds tile row 4 r + j
          const int i = 4 * r + j, m = m0 + screen_row_mixture(i, rpm), row = screen_row_index(i, rpm);
          cl[j * 8 + r] = (m < M) ? -hcP[(size_t)m * 4 + row] : 0.0;
        }
        for (int u = 0; u < 4; ++u) {                        // sub-mixture u of lane group j (u < 4 / rpm)
          const int m = m0 + (4 / rpm) * j + u;
          cl[j * 8 + 4 + u] = (u < 4 / rpm && m < M) ? hlc[m] : -std::numeric_limits<double>::infinity();
        }
      }
    }
  return pq;
}

// the same four rows split into bf16 hi + lo for the screen on the BF16 matrix pipe (gmmmap_layout.hpp, B16; screen16_has(DP))
std::vector<double> pack_screen_bf16(const HostModel &hm) {
  const std::vector<double> &hlc = hm.lc, &hP = hm.P, &hcP = hm.cP;
  const int D = hm.D, DP = hm.DP, M = hm.M;
  const int KSQ = DP / 4, NQ = screen_quads(DP);
  const int STG16 = screen16_stage_doubles(DP), nst16 = screen_stage_count(DP, M, 4);
  std::vector<double> p16((size_t)nst16 * STG16, 0.0);
  const double kEps = 1.0 / 4096.0;                            // 2^-12: see the error bound in gmmmap_layout.hpp
  for (int st = 0; st < nst16; ++st)
    for (int q = 0; q < NQ; ++q) {
      const int m0 = (NQ * st + q) * 4;
      unsigned short *fr = reinterpret_cast<unsigned short *>(&p16[(size_t)st * STG16 + (size_t)q * screen16_tile_doubles()]);
      double *cl = &p16[(size_t)st * STG16 + (size_t)NQ * screen16_tile_doubles() + (size_t)q * 32];
      for (int l = 0; l < 64; ++l) {
        const int r = frag_row(l), gq = frag_col(l), m = m0 + (r >> 2), row = r & 3;     // tile row r <-> mixture r >> 2, screening row r & 3
        unsigned short ph[10] = {0}, pl[10] = {0};             // P[row][feature 4 ks + lane group]; k-steps from KSQ on stay zero
        for (int ks = 0; ks < KSQ; ++ks) split_bf16((m < M && 4 * ks + gq < DP) ? hP[((size_t)m * 4 + row) * DP + 4 * ks + gq] : 0.0, ph[ks], pl[ks]);
        for (int j = 0; j < 8; ++j) {
          fr[(size_t)l * 8 + j] = ph[j];                                     // Ph, k-steps 0..7
          fr[512 + (size_t)l * 8 + j] = pl[j];                               // Pl, k-steps 0..7
        }
        const unsigned short tail[8] = {ph[8], ph[9], ph[8], ph[9], pl[8], pl[9], 0, 0};  // against {xh8, xh9, xl8, xl9, xh8, xh9, 0, 0}
        for (int j = 0; j < 8; ++j) fr[1024 + (size_t)l * 8 + j] = tail[j];
      }
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + j;
        for (int r = 0; r < 4; ++r) {
          const double nrm = (m < M) ? sum_of_squares(&hP[((size_t)m * 4 + r) * DP], D) : 0.0;
          const double c = (m < M) ? hcP[(size_t)m * 4 + r] : 0.0;
          float *cf = reinterpret_cast<float *>(cl + j * 8);          // {c (4 floats) | 2^-12 |P| (4) | 2^-12 |c| (4)}, margins rounded UP
          auto up = [](double v) { return std::nextafterf((float)(v * (1.0 + 0x1p-20)), INFINITY); };
          cf[r] = (float)c;                                           // (its FP32 rounding is inside the 2^-12 |c| margin)
          cf[4 + r] = up(kEps * std::sqrt(nrm));
          cf[8 + r] = up(kEps * std::fabs(c));
        }
        cl[j * 8 + 6] = (m < M) ? hlc[m] : -std::numeric_limits<double>::infinity();
      }
    }
  return p16;
}

// the sixteen strongest rows of every mixture, one tile each, for the second look of that screen (gmmmap_layout.hpp: screen2_*)
std::vector<double> pack_screen2_bf16(const HostModel &hm) {
  const std::vector<double> &hlc = hm.lc, &hP2 = hm.P2, &hcP2 = hm.cP2;
  const int D = hm.D, DP = hm.DP, M = hm.M, R = screen2_rows();
  const int KSQ = DP / 4;
  std::vector<double> p2(screen2_doubles(M), 0.0);
  const double kEps = 1.0 / 4096.0;                            // 2^-12, as pack_screen_bf16
  for (int m = 0; m < M; ++m) {
    unsigned short *fr = reinterpret_cast<unsigned short *>(&p2[(size_t)m * screen2_tile_doubles()]);
    double *cl = &p2[(size_t)m * screen2_tile_doubles() + screen2_const_off()];
    for (int l = 0; l < 64; ++l) {
      const int row = frag_row(l), gq = frag_col(l);           // tile row <-> the mixture's screening row
      unsigned short ph[10] = {0}, pl[10] = {0};
      for (int ks = 0; ks < KSQ; ++ks) split_bf16((4 * ks + gq < DP) ? hP2[((size_t)m * R + row) * DP + 4 * ks + gq] : 0.0, ph[ks], pl[ks]);
      for (int j = 0; j < 8; ++j) {
        fr[(size_t)l * 8 + j] = ph[j];
        fr[512 + (size_t)l * 8 + j] = pl[j];
      }
      const unsigned short tail[8] = {ph[8], ph[9], ph[8], ph[9], pl[8], pl[9], 0, 0};
      for (int j = 0; j < 8; ++j) fr[1024 + (size_t)l * 8 + j] = tail[j];
    }
    for (int j = 0; j < 4; ++j) {                              // lane group j: rows 4 j .. 4 j + 3
      float *cf = reinterpret_cast<float *>(cl + j * 8);
      auto up = [](double v) { return std::nextafterf((float)(v * (1.0 + 0x1p-20)), INFINITY); };
      for (int r = 0; r < 4; ++r) {
        const double nrm = sum_of_squares(&hP2[((size_t)m * R + 4 * j + r) * DP], D), c = hcP2[(size_t)m * R + 4 * j + r];
        cf[r] = (float)c;
        cf[4 + r] = up(kEps * std::sqrt(nrm));
        cf[8 + r] = up(kEps * std::fabs(c));
      }
      cl[j * 8 + 6] = hlc[m];
    }
  }
  return p2;
}

// operand of the frame grouping (gmmmap_group_key_kernel): [-2 mu^x | |mu^x|^2] over its first dimensions, fragment order;
// the last k-step carries |mu|^2 in its first column (rows >= M: 1e300, never the minimum)
std::vector<double> pack_group_keys(const HostModel &hm, const std::vector<double> &hmux) {
  const int D = hm.D, DP = hm.DP, M = hm.M;
  const int KSK = std::min(DP / 4, kGroupKeyDims / 4), KS1 = KSK + 1, MT = (M + 15) / 16, DK = std::min(D, 4 * KSK);
  std::vector<double> gf((size_t)MT * KS1 * 64, 0.0);
  for (int mt = 0; mt < MT; ++mt)
    for (int ks = 0; ks < KS1; ++ks)
      fill_fragment(&gf[((size_t)mt * KS1 + ks) * 64], ks, [&](int row, int k) {
        const int m = 16 * mt + row;
        if (ks < KS1 - 1) return (m < M && k < DK) ? -2.0 * hmux[(size_t)D * m + k] : 0.0;
        if (k != 4 * ks) return 0.0;
        return (m < M) ? sum_of_squares(&hmux[(size_t)D * m], DK) : 1e300;
      });
  return gf;
}

// ... and for the BF16 matrix pipe (gmmmap_group_key16_kernel): -2 mu split into bf16 hi + lo, |mu|^2 as floats
std::vector<double> pack_group_keys_bf16(const HostModel &hm, const std::vector<double> &hmux) {
  const int D = hm.D, DP = hm.DP, M = hm.M;
  const int KSK = std::min(DP / 4, kGroupKeyDims / 4), MT = (M + 15) / 16, DK = std::min(D, 4 * KSK);
  std::vector<double> g16((size_t)MT * (kKey16TileBytes / 8), 0.0);
  for (int mt = 0; mt < MT; ++mt) {
    unsigned short *hi = reinterpret_cast<unsigned short *>(&g16[(size_t)mt * (kKey16TileBytes / 8)]), *lo = hi + 512;
    float *msq = reinterpret_cast<float *>(hi + 1024);
    for (int l = 0; l < 64; ++l) {
      const int m = 16 * mt + frag_row(l), gq = frag_col(l);
      for (int j = 0; j < 8; ++j) {
        const int k = 4 * j + gq;
        const double v = (m < M && j < KSK && k < DK) ? -2.0 * hmux[(size_t)D * m + k] : 0.0;
        split_bf16(v, hi[(size_t)l * 8 + j], lo[(size_t)l * 8 + j]);
      }
    }
    for (int r = 0, m = 16 * mt; r < 16; ++r, ++m)            // lane group r >> 2 reads floats 4 (r >> 2) .. + 3
      msq[r] = (float)((m < M) ? sum_of_squares(&hmux[(size_t)D * m], DK) : 1e30);
  }
  return g16;
}

// A transposed, [M][DP (k)][DP (row)]: what convert_from_logdens_kernel reads
std::vector<double> transpose_A(const HostModel &hm) {
  const int DP = hm.DP, M = hm.M;
  const size_t pp = (size_t)DP * DP;
  std::vector<double> hAt(hm.A.size());
  for (int m = 0; m < M; ++m)
    for (int r = 0; r < DP; ++r)
      for (int k = 0; k < DP; ++k) hAt[pp * m + (size_t)k * DP + r] = hm.A[pp * m + (size_t)r * DP + k];
  return hAt;
}

// ------------------------------------------------------------------------------------------------
// the sequence, and the p(x) handles of estep_full.hip and gmm_em.hip
// ------------------------------------------------------------------------------------------------
int gmmmap_prepare(vcmi_gmmmap *g, const double *w, const double *mu, const double *sigma, int Dj, int M, int swap, bool px_only) {
  HostModel hm;
  VCMI_TRY(factor_model(g, hm, w, mu, sigma, Dj, M, swap, px_only));
  const int D = g->D = hm.D, DP = g->DP = hm.DP;
  g->M = M;
  const bool tiles = gmmmap_has_mfma(DP);       // the tile kernel reads the packed blocks, every other kernel the row-major ones
  if (!px_only) g->model = profile_model(hm, g->h_mux, w);
  // row-major blocks for the generic kernels; a p(x)-only handle that takes the MFMA path needs only its packed blocks
  if (!(px_only && tiles)) {
    VCMI_TRY(upload_now(g->U, hm.U));
    VCMI_TRY(upload_now(g->cz, hm.cz));
    VCMI_TRY(upload_now(g->lc, hm.lc));
  }
  if (!px_only) {
    VCMI_TRY(upload_now(g->A, hm.A));
    VCMI_TRY(upload_now(g->b, hm.b));
    if (!tiles && D > 16 && D <= 160) VCMI_TRY(upload_now(g->At, transpose_A(hm)));
  }
  if (tiles) {
    if (!px_only) VCMI_TRY(upload_now(g->packed, pack_tiles(hm, 0)));
    VCMI_TRY(upload_now(g->packedU, pack_tiles(hm, 1)));
    VCMI_TRY(upload_now(g->packedU2, pack_tiles(hm, 2)));
  }
  // the screens exist where factor_model() made their rows: a joint model with a tile kernel, D >= 4, M <= 1024
  if (!hm.P.empty() && screen_has_kernel(DP)) {       // fvconvert's (shape 3)
    int rpm = choose_screen_rows(g->model, DP, M);
    if (debug_flag(kDbgScreenRows4)) rpm = 4;        // (test hooks, read when the converter is CREATED)
    if (debug_flag(kDbgScreenRows2)) rpm = 2;
    if (debug_flag(kDbgScreenRows1)) rpm = 1;
    g->screen_rpm = rpm;
    g->model_undecided4_frac = g->model.undecided_rows[rpm == 4 ? 0 : rpm == 2 ? 1 : 2];     // what the chosen screen lets through
    VCMI_TRY(upload_now(g->packedQ, pack_screen(hm, rpm)));
    if (rpm == 4 && screen16_has(DP)) {
      VCMI_TRY(upload_now(g->packedQ16, pack_screen_bf16(hm)));
      VCMI_TRY(upload_now(g->packedQ2, pack_screen2_bf16(hm)));
    }
  }
  // the group radius of that screen: the table, lmin for the handle's prune, and whether this model's own frames stay inside
  g->radius = ScreenRadius{};
  g->radius_on = false;
  g->radius_pass_frac = 0.0;
  if (!hm.Sxx.empty() && g->packedQ.p) {
    g->radius = screen_radius_table(hm, g->h_mux);
    std::vector<double> R, lmin;
    screen_radius_lmin(g->radius, g->prune, R, lmin);
    g->radius_pass_frac = screen_radius_pass_frac(g->model, g->radius, lmin);
    g->radius_on = choose_screen_radius(g->radius_pass_frac);
    VCMI_TRY(upload_now(g->lmin, lmin));
  }
  // ... and predict's (gmmmap_screen_argmax_kernel): always four rows per mixture, every tile-kernel dimension
  if (!hm.P.empty()) VCMI_TRY(upload_now(g->packedQA, pack_screen(hm, 4)));
  if (!g->h_mux.empty()) {                            // fvconvert's frame grouping (made for every handle, p(x)-only ones too)
    VCMI_TRY(upload_now(g->gfrag, pack_group_keys(hm, g->h_mux)));
    VCMI_TRY(upload_now(g->gfrag16, pack_group_keys_bf16(hm, g->h_mux)));
  }
  return VCMI_OK;
}

int gmm_px_handle_here(vcmi_gmmmap **inout) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (*inout && (*inout)->device != dev) {
    delete *inout;
    *inout = nullptr;
  }
  if (!*inout) *inout = new (std::nothrow) vcmi_gmmmap();
  if (!*inout) return fail(VCMI_ERR_OOM, "out of host memory");
  (*inout)->bind_device(dev);
  return VCMI_OK;
}

int gmm_px_create(const double *w, const double *mu, const double *sigma, int D, int M, vcmi_gmmmap **inout) {
  VCMI_TRY(check_device());
  VCMI_TRY(gmm_px_handle_here(inout));
  const int rc = gmmmap_prepare(*inout, w, mu, sigma, D, M, 0, /*px_only=*/true);
  if (rc != VCMI_OK) {
    delete *inout;
    *inout = nullptr;
  }
  return rc;
}

}  // namespace vcmi

// Test hook, deliberately absent from include/vcmi.h (like vcmi_debug_force): the group radius of a joint model on the host
// alone -- no device, no handle.  c (M * M * J, may be NULL): the table, NaN where there is no bound; R, lmin (M each): the
// radii less their rounding margin and lc_g - R_g / 2 for `prune` (any value: vcmi_gmmmap_set_prune's floor of 40 is not this
// function's business); *pass_frac (may be NULL): the share of the model's 256 profile frames inside their mixture's radius.
extern "C" int vcmi_debug_screen_radius(const double *w, const double *mu, const double *sigma, int Dj, int M, int swap, double prune,
                                        double *c, double *R, double *lmin, double *pass_frac) {
  using namespace vcmi;
  if (!w || !mu || !sigma || !R || !lmin) return fail(VCMI_ERR_ARG, "vcmi_debug_screen_radius: NULL argument");
  if (Dj < 2 || (Dj & 1) || M < 1) return fail(VCMI_ERR_DIM, "vcmi_debug_screen_radius: joint dimension %d / mixtures %d invalid", Dj, M);
  vcmi_gmmmap g;
  HostModel hm;
  VCMI_TRY(factor_model(&g, hm, w, mu, sigma, Dj, M, swap, false));
  if (hm.Sxx.empty()) return fail(VCMI_ERR_ARG, "vcmi_debug_screen_radius: no group radius for dimension %d, %d mixtures", Dj / 2, M);
  const ScreenRadius rt = screen_radius_table(hm, g.h_mux);
  std::vector<double> Rv, lv;
  screen_radius_lmin(rt, prune, Rv, lv);
  if (c) memcpy(c, rt.c.data(), rt.c.size() * sizeof(double));
  memcpy(R, Rv.data(), (size_t)M * sizeof(double));
  memcpy(lmin, lv.data(), (size_t)M * sizeof(double));
  if (pass_frac) *pass_frac = screen_radius_pass_frac(profile_model(hm, g.h_mux, w), rt, lv);
  return VCMI_OK;
}

// diffgmm(params) -- src/diffgmm.jl:9-25, on the joint parameters mu (2D,M), sigma (2D,2D,M) (host arithmetic: a
// one-time parameter transform).  Feed the result to vcmi_gmmmap_create for the differential converter.
extern "C" int vcmi_diffgmm(const double *mu, const double *sigma, int Dj, int M, double *mu_out, double *sigma_out) {
  if (!mu || !sigma || !mu_out || !sigma_out) return vcmi::fail(VCMI_ERR_ARG, "vcmi_diffgmm: NULL argument");
  if (Dj < 2 || (Dj & 1) || M < 1) return vcmi::fail(VCMI_ERR_DIM, "vcmi_diffgmm: joint dimension %d / mixtures %d invalid", Dj, M);
  const int D = Dj / 2;
  for (int m = 0; m < M; ++m) {
    const double *S = sigma + (size_t)Dj * Dj * m;
    double *O = sigma_out + (size_t)Dj * Dj * m;
    for (int d = 0; d < D; ++d) {
      const double mx = mu[d + (size_t)Dj * m], my = mu[D + d + (size_t)Dj * m];
      mu_out[d + (size_t)Dj * m] = mx;
      mu_out[D + d + (size_t)Dj * m] = my - mx;                                  // eq. (6)
    }
    for (int c = 0; c < D; ++c)
      for (int r = 0; r < D; ++r) {
        const double xx = S[r + (size_t)Dj * c], xy = S[r + (size_t)Dj * (D + c)], yx = S[(D + r) + (size_t)Dj * c],
                     yy = S[(D + r) + (size_t)Dj * (D + c)];
        O[r + (size_t)Dj * c] = xx;
        O[r + (size_t)Dj * (D + c)] = xy - xx;                                    // eq. (7)
        O[(D + c) + (size_t)Dj * r] = xy - xx;                                    // its transpose
        O[(D + r) + (size_t)Dj * (D + c)] = xx + yy - xy - yx;                    // eq. (8)
      }
  }
  return VCMI_OK;
}
