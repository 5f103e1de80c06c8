// traj_diag_prepare_check.cpp -- the host arithmetic of the diagonal model of a TrajectoryGMMMap (traj_prepare_diag,
// csrc/traj_prepare.cpp) on the CPU: exact facts about q and the three images of diag(q_m) at static D = 3, 12 and 47, M = 2, and
// the refusal of a conditional variance that is zero, negative or not a number.  Built by tests/test_traj_diag_host.py with
// -fsanitize=address,undefined, so a packer that reads or writes past an image is a finding as well.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../voiceconversion.jl_amd/csrc/gmmmap_layout.hpp"
#include "../../voiceconversion.jl_amd/csrc/traj_prepare.hpp"
#include "../../voiceconversion.jl_amd/csrc/vcmi_common.hpp"

using namespace vcmi;

static int bad = 0;
static int curD = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      if (++bad <= 20) printf("traj_diag_prepare_check: D=%d: %s (line %d)\n", curD, #cond, __LINE__); \
    }                                                                                \
  } while (0)

struct Lcg {      // deterministic uniform deviates in (-1, 1)
  unsigned long long s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((s >> 11) & ((1ull << 53) - 1)) * (2.0 / 9007199254740992.0) - 1.0;
  }
};

struct Inputs {
  std::vector<double> A, Sxy, Syy;
};

// A and Sxy small and dense, Syy symmetric and diagonally dominant: every conditional variance is near D2 + 1
static Inputs make_inputs(int D2, int M, unsigned long long seed) {
  Lcg g{seed};
  const size_t nn = (size_t)D2 * D2;
  Inputs in;
  in.A.resize(nn * M);
  in.Sxy.resize(nn * M);
  in.Syy.assign(nn * M, 0.0);
  for (auto &v : in.A) v = 0.3 * g.next();
  for (auto &v : in.Sxy) v = 0.1 * g.next();
  for (int m = 0; m < M; ++m)
    for (int r = 0; r < D2; ++r) {
      for (int c = 0; c < r; ++c) in.Syy[nn * m + (size_t)r * D2 + c] = in.Syy[nn * m + (size_t)c * D2 + r] = 0.2 * g.next();
      in.Syy[nn * m + (size_t)r * D2 + r] = D2 + 1.0 + g.next();
    }
  return in;
}

// diagonal r of the conditional covariance of mixture m, in long double: Syy[r,r] - sum_k A[r,k] Sxy[k,r]
static long double cond_var(const Inputs &in, int D2, int m, int r, long double *mag) {
  const size_t nn = (size_t)D2 * D2;
  long double s = in.Syy[nn * m + (size_t)r * D2 + r], a = fabsl(s);
  for (int k = 0; k < D2; ++k) {
    const long double p = (long double)in.A[nn * m + (size_t)r * D2 + k] * in.Sxy[nn * m + (size_t)k * D2 + r];
    s -= p;
    a += fabsl(p);
  }
  *mag = a;
  return s;
}

static void check_dim(int D) {
  curD = D;
  const int D2 = 2 * D, M = 2, NT = (D2 + 15) / 16, KS = (D2 + 3) / 4;
  const size_t nn = (size_t)D2 * D2;
  const Inputs in = make_inputs(D2, M, 7654321ull + D);
  TrajDiagModel dm;
  CHECK(traj_prepare_diag(in.A, in.Sxy, in.Syy, D2, M, dm) == VCMI_OK);
  CHECK(dm.q.size() == (size_t)D2 * M && dm.Q.size() == nn * M && dm.QT.size() == nn * M);
  CHECK(dm.Qfrag.size() == (size_t)M * NT * KS * 64);
  if (bad) return;
  // q_m diag(C_m) == 1 to rounding: the sum of D2 + 1 terms in double (error <= (D2 + 2) eps sum |terms|), one division
  const double eps = std::numeric_limits<double>::epsilon();
  for (int m = 0; m < M; ++m)
    for (int r = 0; r < D2; ++r) {
      long double mag;
      const long double c = cond_var(in, D2, m, r, &mag);
      const long double one = (long double)dm.q[(size_t)D2 * m + r] * c;
      CHECK(dm.q[(size_t)D2 * m + r] > 0.0);
      CHECK(fabsl(one - 1.0L) <= (D2 + 4) * eps * (double)(mag / c));
    }
  // the images are the fills of diag(q_m): row-major, transposed, and fragment by fragment with every other slot exactly 0
  std::vector<char> used(dm.Qfrag.size(), 0);
  for (int m = 0; m < M; ++m)
    for (int r = 0; r < D2; ++r)
      for (int k = 0; k < D2; ++k) {
        const double want = r == k ? dm.q[(size_t)D2 * m + r] : 0.0;
        CHECK(dm.Q[nn * m + (size_t)r * D2 + k] == want);
        CHECK(dm.QT[nn * m + (size_t)k * D2 + r] == want);
        int lane = -1;
        for (int l = 0; l < 64; ++l)
          if (frag_row(l) == r % 16 && frag_col(l) == k % 4) lane = l;
        const size_t pos = (((size_t)m * NT + r / 16) * KS + k / 4) * 64 + lane;
        CHECK(lane >= 0 && dm.Qfrag[pos] == want);
        if (r != k) CHECK(dm.Qfrag[pos] == 0.0 && !std::signbit(dm.Qfrag[pos]));     // off-diagonal slots: exactly +0
        used[pos] = 1;
      }
  for (size_t i = 0; i < dm.Qfrag.size(); ++i)
    if (!used[i]) CHECK(dm.Qfrag[i] == 0.0);
  // the fragment image agrees with the full model's packer: traj_prepare_model on inputs whose conditional covariance IS
  // diag(1 / q) packs inv(diag(1 / q)) -- the same matrix up to the rounding of two reciprocals -- at the same slots
  {
    Inputs z;
    z.A.assign(nn * M, 0.0);
    z.Sxy.assign(nn * M, 0.0);
    z.Syy.assign(nn * M, 0.0);
    for (int m = 0; m < M; ++m)
      for (int r = 0; r < D2; ++r) z.Syy[nn * m + (size_t)r * D2 + r] = 1.0 / dm.q[(size_t)D2 * m + r];
    std::vector<double> mu((size_t)D2 * M, 0.0);
    TrajModel tm;
    CHECK(traj_prepare_model(z.A, z.Sxy, z.Syy, mu, mu, D2, M, tm) == VCMI_OK);
    CHECK(tm.NT == NT && tm.KS == KS && tm.Qfrag.size() == dm.Qfrag.size());
    for (size_t i = 0; i < dm.Qfrag.size() && i < tm.Qfrag.size(); ++i) {
      CHECK((tm.Qfrag[i] == 0.0) == (dm.Qfrag[i] == 0.0));
      CHECK(std::fabs(tm.Qfrag[i] - dm.Qfrag[i]) <= 4 * eps * std::fabs(dm.Qfrag[i]));
    }
  }
  // a zero, a negative and a NaN conditional variance, in the last slot of the last mixture
  const size_t last = nn * (M - 1) + nn - 1;
  const double keep = in.Syy[last];
  long double mag;
  const double rest = (double)(keep - cond_var(in, D2, M - 1, D2 - 1, &mag));     // sum_k A[r,k] Sxy[k,r]
  for (double v : {rest, rest - 1.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
    Inputs b = in;
    b.Syy[last] = v;
    TrajDiagModel d2;
    if (v == rest) {      // (the device of the exact zero: A = 0 in that row, Syy = 0)
      for (int k = 0; k < D2; ++k) b.A[nn * (M - 1) + (size_t)(D2 - 1) * D2 + k] = 0.0;
      b.Syy[last] = 0.0;
    }
    CHECK(traj_prepare_diag(b.A, b.Sxy, b.Syy, D2, M, d2) == VCMI_ERR_NOT_PD);
  }
}

int main() {
  check_dim(3);
  check_dim(12);
  check_dim(47);
  if (bad) {
    printf("traj_diag_prepare_check: %d checks failed\n", bad);
    return 1;
  }
  printf("traj_diag_prepare_check: ok\n");
  return 0;
}
