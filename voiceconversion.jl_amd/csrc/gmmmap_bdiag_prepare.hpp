// gmmmap_bdiag_prepare.hpp -- host preparation of the cross-diagonal frame-by-frame converter (vcmi_bdmap, gmmmap_bdiag.hip):
// from the parameters train_gmm(covariance_type="block_diag") returns, the table the convert kernel reads.  No HIP call and
// no device type: tests/c/gmmmap_bdiag_prepare_check.cpp checks it with a plain C++ compiler.
#pragma once
#include <cstdint>
#include <vector>

namespace vcmi {

constexpr int kBdmapMaxD = 128, kBdmapMaxM = 256;   // what the cross-diagonal training can produce (estep_internal.hpp)
constexpr int kBdmapPrm1 = 2;                       // doubles per (mixture, dimension) of the log-density table
constexpr int kBdmapPrm3 = 4;                       // ... and of the regression table
constexpr int kBdmapPrm4 = 4;                       // ... and of the trajectory table

struct BdmapTable {
  int D = 0, DP = 0, M = 0;        // DP: D rounded up to a multiple of 4 (the log-density pass takes four dimensions at once)
  // of the SOURCE side x and the TARGET side y (after the swap); rows d >= D are zeros.  Two tables, one per pass of the
  // kernel, each contiguous over d so that a pass fetches several dimensions of a mixture with one wide scalar load:
  // prm1[(m DP + d) 2 + .] = [mu_x, 1 / v_x]
  // prm3[(m DP + d) 4 + .] = [mu_x, a = c / v_x, mu_y, 0]
  std::vector<double> prm1, prm3;
  // cst[m] = log w_m - (D log 2 pi + sum_d log v_x) / 2, the sum over d = 0 .. D-1 in that order with a compensated
  // (Neumaier) accumulator; -infinity for w_m <= 0
  std::vector<double> cst;
  std::vector<double> a;           // (D,M), dimension fastest: vcmi_bdmap_get_a
  // What trajectory conversion straight from the model reads (vcmi_traj_create_bdiag); the frame-by-frame
  // passes read none of it.  The conditional covariance of a cross-diagonal model is diagonal exactly:
  // q[d + D m] = 1 / fma(-a, c, v_y), the reciprocal conditional variance, (D,M) dimension fastest -- the [M][2 D_static]
  // table the tridiagonal solver indexes (traj_diag.hip);
  // prm4[(m DP + d) 4 + .] = [mu_x, a, mu_y, q], one 32-byte row per (mixture, dimension) for the per-frame gather of the
  // fused arg-max + g_t pass; rows d >= D are zeros.
  // q_bad: index d + D m of the first pair in memory order whose conditional variance is zero, negative or not finite in
  // FP64 (a valid pair can round there: |c| within an ulp of sqrt(v_x v_y)), -1: none.  The entries of such a pair hold what
  // the division gave.
  std::vector<double> q, prm4;
  int64_t q_bad = -1;
};

// weights (M), mu (Dj,M), covars (Dj + D, M) = [variances of the Dj rows | D pair cross-covariances], D = Dj / 2 (the caller
// has checked Dj even, 1 <= D <= kBdmapMaxD, 1 <= M <= kBdmapMaxM).  swap: source = rows D .. Dj-1 (src/gmmmap.jl:74-78).
// Returns -1 and fills *out, or the index d + D m of the first invalid pair in memory order (first_bad_pair: a pair's validity
// does not depend on the swap) and leaves *out alone.
int64_t bdmap_prepare(const double *weights, const double *mu, const double *covars, int Dj, int M, bool swap, BdmapTable *out);

}  // namespace vcmi
