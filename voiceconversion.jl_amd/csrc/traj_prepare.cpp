// traj_prepare.cpp -- see traj_prepare.hpp.
#include "traj_prepare.hpp"

#include <cmath>

#include "vcmi_common.hpp"
#include "host_linalg.hpp"
#include "gmmmap_layout.hpp"

namespace vcmi {

static constexpr double kEmLog2Pi = 1.8378770664093454835606594728112;

// W [M][D2][D2] row-major -> F [M][NT][KS][64]: tile (i, ks) of every matrix in MFMA A-operand order, zero outside the matrix
static void pack_fragments(const std::vector<double> &W, int D2, int M, std::vector<double> &F) {
  const int NT = (D2 + 15) / 16, KS = (D2 + 3) / 4;
  const size_t nn = (size_t)D2 * D2;
  F.assign((size_t)M * NT * KS * 64, 0.0);
  for (int m = 0; m < M; ++m)
    for (int i = 0; i < NT; ++i)
      for (int ks = 0; ks < KS; ++ks)
        fill_fragment(&F[(((size_t)m * NT + i) * KS + ks) * 64], ks, [&](int row, int k) {
          return (16 * i + row < D2 && k < D2) ? W[nn * m + (size_t)(16 * i + row) * D2 + k] : 0.0;
        });
}
// Q [M][D2][D2] row-major -> its transposes
static void transpose_blocks(const std::vector<double> &Q, int D2, int M, std::vector<double> &QT) {
  const size_t nn = (size_t)D2 * D2;
  QT.assign(nn * M, 0.0);
  for (int m = 0; m < M; ++m)
    for (int r = 0; r < D2; ++r)
      for (int k = 0; k < D2; ++k) QT[nn * m + (size_t)k * D2 + r] = Q[nn * m + (size_t)r * D2 + k];
}

int traj_prepare_diag(const std::vector<double> &h_A, const std::vector<double> &h_Sxy, const std::vector<double> &h_Syy, int D2,
                      int M, TrajDiagModel &dm) {
  const size_t nn = (size_t)D2 * D2;
  dm.q.assign((size_t)D2 * M, 0.0);
  dm.Q.assign(nn * M, 0.0);
  std::vector<double> tmp(nn);
  for (int m = 0; m < M; ++m) {
    la::matmul(&h_A[nn * m], &h_Sxy[nn * m], D2, tmp.data());     // the product traj_prepare_model inverts, diagonal kept
    for (int r = 0; r < D2; ++r) {
      const double c = h_Syy[nn * m + (size_t)r * D2 + r] - tmp[(size_t)r * D2 + r];
      const double q = 1.0 / c;
      if (!(q > 0.0) || !std::isfinite(q))     // c zero, negative, NaN, or beyond either end of the range
        return fail(VCMI_ERR_NOT_PD, "TrajectoryGMMMap: conditional variance %d of mixture %d is not positive", r + 1, m + 1);
      dm.q[(size_t)D2 * m + r] = q;
      dm.Q[nn * m + (size_t)r * D2 + r] = q;
    }
  }
  transpose_blocks(dm.Q, D2, M, dm.QT);
  pack_fragments(dm.Q, D2, M, dm.Qfrag);
  return VCMI_OK;
}

int traj_prepare_model(const std::vector<double> &h_A, const std::vector<double> &h_Sxy, const std::vector<double> &h_Syy,
                       const std::vector<double> &h_mux, const std::vector<double> &h_muy, int D2, int M, TrajModel &tm) {
  const int D = D2 / 2;
  const size_t nn = (size_t)D2 * D2;
  std::vector<double> &Q = tm.Q, &QT = tm.QT, &AT = tm.AT, &bv = tm.b;
  Q.assign(nn * M, 0.0);
  bv.assign((size_t)D2 * M, 0.0);
  std::vector<double> tmp(nn), S(nn);
  for (int m = 0; m < M; ++m) {
    // Dy_m = inv(Syy_m - A_m Sxy_m), src/trajectory_gmmmap.jl:24-28
    la::matmul(&h_A[nn * m], &h_Sxy[nn * m], D2, tmp.data());
    for (size_t k = 0; k < nn; ++k) S[k] = h_Syy[nn * m + k] - tmp[k];
    if (!la::inverse(S.data(), D2, &Q[nn * m]))
      return fail(VCMI_ERR_NOT_PD, "TrajectoryGMMMap: conditional covariance of mixture %d is singular", m + 1);
    for (int r = 0; r < D2; ++r) {
      double ba = 0.0;
      for (int k = 0; k < D2; ++k) ba += h_A[nn * m + (size_t)r * D2 + k] * h_mux[(size_t)D2 * m + k];
      bv[(size_t)D2 * m + r] = h_muy[(size_t)D2 * m + r] - ba;
    }
  }
  transpose_blocks(Q, D2, M, QT);
  transpose_blocks(h_A, D2, M, AT);
  // c_m = logdet((Q_m + Q_m') / 2) / 2 of the EM objective (traj_em.hip), with its constant - D log 2 pi; a model without it
  // (some symmetrised Q_m not positive definite) converts as before and refuses vcmi_traj_set_em(t, n > 0)
  tm.cm.assign((size_t)M, 0.0);
  tm.em_pd = true;
  for (int m = 0; m < M && tm.em_pd; ++m) {
    for (int r = 0; r < D2; ++r)
      for (int c = 0; c < D2; ++c) S[(size_t)r * D2 + c] = 0.5 * (Q[nn * m + (size_t)r * D2 + c] + Q[nn * m + (size_t)c * D2 + r]);
    if (!la::cholesky_from_upper(S.data(), D2, tmp.data())) {
      tm.em_pd = false;
      break;
    }
    double ld = 0.0;
    for (int r = 0; r < D2; ++r) ld += std::log(tmp[(size_t)r * D2 + r]);     // = logdet / 2
    tm.cm[(size_t)m] = ld - (double)D * kEmLog2Pi;
  }
  // Q and A in MFMA A-operand order: fragment (row tile i, k-step ks) holds rows 16 i .. 16 i + 15, columns 4 ks .. 4 ks + 3
  tm.NT = (D2 + 15) / 16;
  tm.KS = (D2 + 3) / 4;
  pack_fragments(Q, D2, M, tm.Qfrag);
  pack_fragments(h_A, D2, M, tm.Afrag);
  // Static dimensions without an instantiation of the blocked solver run in the next larger one
  tm.Dpad = traj_blk_padded_dim(D);
  tm.Qpad.clear();
  if (tm.Dpad) {
    const int Dp = tm.Dpad, Dp2 = 2 * Dp;
    tm.Qpad.assign((size_t)M * Dp2 * Dp2, 0.0);
    for (int m = 0; m < M; ++m) {
      double *q = &tm.Qpad[(size_t)m * Dp2 * Dp2];
      for (int r = 0; r < D2; ++r)
        for (int c = 0; c < D2; ++c) {
          const int rp = (r / D) * Dp + r % D, cp = (c / D) * Dp + c % D;     // [static ; delta] halves keep their blocks
          q[(size_t)rp * Dp2 + cp] = Q[nn * m + (size_t)r * D2 + c];
        }
      for (int d = D; d < Dp; ++d) q[(size_t)d * Dp2 + d] = 1.0;              // padding: P = I, r = 0 -> y = 0, decoupled
    }
  }
  return VCMI_OK;
}

}  // namespace vcmi
