// traj_prepare.hpp -- the host arithmetic of the TrajectoryGMMMap constructor (reference src/trajectory_gmmmap.jl:11-31): from
// the host copies a vcmi_gmmmap keeps to every image vcmi_traj_create uploads.  No handle, no device: it also runs in the
// CPU sanitizer build (tests/c/traj_prepare_check.cpp).
#pragma once
#include <vector>

// The static dimensions the blocked solver (traj_solve_blk.hpp) is instantiated for.  The one list: the dispatch of
// traj_solve.hip expands it, and so do the two questions below.
#define VCMI_TRAJ_BLK_DIMS(X) X(12) X(16) X(20) X(24) X(25) X(30) X(32) X(40) X(46)

namespace vcmi {

inline bool traj_blk_has(int D) {
#define VCMI_TRAJ_BLK_IS(DV) if (D == DV) return true;
  VCMI_TRAJ_BLK_DIMS(VCMI_TRAJ_BLK_IS)
#undef VCMI_TRAJ_BLK_IS
  return false;
}
// the instantiation a static dimension without its own runs in; 0: none (46 is the largest whose window fits the LDS)
inline int traj_blk_padded_dim(int D) {
  for (int d = D; d <= 46 && !traj_blk_has(D); ++d)
    if (traj_blk_has(d)) return d;
  return 0;
}

struct TrajModel {
  int NT = 0, KS = 0;                // row tiles / k-steps of the fragment images
  int Dpad = 0;                      // traj_blk_padded_dim(D)
  bool em_pd = false;                // (Q_m + Q_m') / 2 positive definite for every m: c_m exists
  std::vector<double> Q, QT, AT;     // [M][2D][2D] row-major Q_m = Dy_m; Q_m' and A_m'
  std::vector<double> b;             // [M][2D] mu^y_m - A_m mu^x_m
  std::vector<double> Qfrag, Afrag;  // Q and A in MFMA A-operand order [M][NT][KS][64] (fill_fragment, gmmmap_layout.hpp)
  std::vector<double> cm;            // [M] logdet((Q_m + Q_m') / 2) / 2 - D log 2 pi; zeros from the first m without one
  std::vector<double> Qpad;          // [M][2 Dpad][2 Dpad]: Q with the extra static dimensions decoupled; empty when Dpad = 0
};
// h_A, h_Sxy, h_Syy: [M][D2][D2] row-major; h_mux, h_muy: [M][D2].  VCMI_ERR_NOT_PD: some Syy_m - A_m Sxy_m is singular.
int traj_prepare_model(const std::vector<double> &h_A, const std::vector<double> &h_Sxy, const std::vector<double> &h_Syy,
                       const std::vector<double> &h_mux, const std::vector<double> &h_muy, int D2, int M, TrajModel &tm);

// The second model of a converter (VCMI_TRAJ_PRECISION_DIAG): the conditional covariance C_m = Syy_m - A_m Sxy_m taken as
// diagonal, q_m = 1 ./ diag(C_m) -- the reciprocals of the conditional variances, NOT the diagonal of Q_m = inv(C_m).  The g_t
// kernels run unchanged on the images of diag(q_m), packed by the routines that pack Q_m; the tridiagonal solver
// (traj_diag.hip) reads q itself.
struct TrajDiagModel {
  std::vector<double> q;             // [M][2D]
  std::vector<double> Q, QT;         // [M][2D][2D] diag(q_m), row-major and transposed (the same bytes)
  std::vector<double> Qfrag;         // diag(q_m) in MFMA A-operand order [M][NT][KS][64]
};
// VCMI_ERR_NOT_PD: some conditional variance is zero, negative or not finite.
int traj_prepare_diag(const std::vector<double> &h_A, const std::vector<double> &h_Sxy, const std::vector<double> &h_Syy, int D2,
                      int M, TrajDiagModel &dm);

}  // namespace vcmi
