// traj_prepare_check.cpp -- the host arithmetic of the TrajectoryGMMMap constructor (csrc/traj_prepare.cpp) on the CPU: exact
// facts about every image vcmi_traj_create uploads, at static D = 3 (runs padded in the instantiation for 12), D = 12 (has its
// own) and D = 47 (beyond the blocked solver), M = 2.  Built by tests/test_traj_prepare_host.py with
// -fsanitize=address,undefined, so a packer that reads or writes past an image is a finding as well.
#include <cstdio>
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
      if (++bad <= 20) printf("traj_prepare_check: D=%d: %s (line %d)\n", curD, #cond, __LINE__); \
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
  std::vector<double> A, Sxy, Syy, mux, muy;
};

// A and Sxy small and dense, Syy symmetric and diagonally dominant: Syy - A Sxy is well conditioned and Q_m close to SPD
static Inputs make_inputs(int D2, int M, unsigned long long seed) {
  Lcg g{seed};
  const size_t nn = (size_t)D2 * D2;
  Inputs in;
  in.A.resize(nn * M);
  in.Sxy.resize(nn * M);
  in.Syy.assign(nn * M, 0.0);
  in.mux.resize((size_t)D2 * M);
  in.muy.resize((size_t)D2 * M);
  for (auto &v : in.A) v = 0.3 * g.next();
  for (auto &v : in.Sxy) v = 0.1 * g.next();
  for (auto &v : in.mux) v = g.next();
  for (auto &v : in.muy) v = g.next();
  for (int m = 0; m < M; ++m)
    for (int r = 0; r < D2; ++r) {
      for (int c = 0; c < r; ++c) in.Syy[nn * m + (size_t)r * D2 + c] = in.Syy[nn * m + (size_t)c * D2 + r] = 0.2 * g.next();
      in.Syy[nn * m + (size_t)r * D2 + r] = D2 + 1.0 + g.next();
    }
  return in;
}

// every element of the row-major W [M][D2][D2] at its fragment slot, every other slot zero
static void check_fragments(const std::vector<double> &F, const std::vector<double> &W, int D2, int M, int NT, int KS) {
  CHECK(F.size() == (size_t)M * NT * KS * 64);
  if (F.size() != (size_t)M * NT * KS * 64) return;
  std::vector<char> used(F.size(), 0);
  for (int m = 0; m < M; ++m)
    for (int r = 0; r < D2; ++r)
      for (int k = 0; k < D2; ++k) {
        int lane = -1;
        for (int l = 0; l < 64; ++l)
          if (frag_row(l) == r % 16 && frag_col(l) == k % 4) lane = l;
        const size_t pos = (((size_t)m * NT + r / 16) * KS + k / 4) * 64 + lane;
        CHECK(lane >= 0 && F[pos] == W[((size_t)m * D2 + r) * D2 + k]);
        used[pos] = 1;
      }
  for (size_t i = 0; i < F.size(); ++i)
    if (!used[i]) CHECK(F[i] == 0.0);
}

static void check_dim(int D, int expect_dpad) {
  curD = D;
  const int D2 = 2 * D, M = 2;
  const size_t nn = (size_t)D2 * D2;
  const Inputs in = make_inputs(D2, M, 1234567ull + D);
  TrajModel tm;
  CHECK(traj_prepare_model(in.A, in.Sxy, in.Syy, in.mux, in.muy, D2, M, tm) == VCMI_OK);
  CHECK(tm.Q.size() == nn * M && tm.QT.size() == nn * M && tm.AT.size() == nn * M && tm.b.size() == (size_t)D2 * M);
  CHECK(tm.cm.size() == (size_t)M);
  CHECK(tm.NT == (D2 + 15) / 16 && tm.KS == (D2 + 3) / 4);
  CHECK(tm.em_pd);
  if (bad) return;
  // transposes, and b = mu^y - A mu^x accumulated over k in order
  for (int m = 0; m < M; ++m)
    for (int r = 0; r < D2; ++r) {
      double ba = 0.0;
      for (int k = 0; k < D2; ++k) {
        CHECK(tm.QT[nn * m + (size_t)k * D2 + r] == tm.Q[nn * m + (size_t)r * D2 + k]);
        CHECK(tm.AT[nn * m + (size_t)k * D2 + r] == in.A[nn * m + (size_t)r * D2 + k]);
        ba += in.A[nn * m + (size_t)r * D2 + k] * in.mux[(size_t)D2 * m + k];
      }
      CHECK(tm.b[(size_t)D2 * m + r] == in.muy[(size_t)D2 * m + r] - ba);
    }
  check_fragments(tm.Qfrag, tm.Q, D2, M, tm.NT, tm.KS);
  check_fragments(tm.Afrag, in.A, D2, M, tm.NT, tm.KS);
  // the padded dimension and the padded precision matrices
  CHECK(tm.Dpad == expect_dpad);
  CHECK(tm.Dpad == traj_blk_padded_dim(D));
  if (tm.Dpad == 0) {
    CHECK(tm.Qpad.empty());
    return;
  }
  const int Dp = tm.Dpad, Dp2 = 2 * Dp;
  CHECK(tm.Qpad.size() == (size_t)M * Dp2 * Dp2);
  if (tm.Qpad.size() != (size_t)M * Dp2 * Dp2) return;
  for (int m = 0; m < M; ++m) {
    std::vector<double> want((size_t)Dp2 * Dp2, 0.0);
    for (int r = 0; r < D2; ++r)
      for (int c = 0; c < D2; ++c) want[(size_t)((r / D) * Dp + r % D) * Dp2 + (c / D) * Dp + c % D] = tm.Q[nn * m + (size_t)r * D2 + c];
    for (int d = D; d < Dp; ++d) want[(size_t)d * Dp2 + d] = 1.0;      // padding rows of the static half
    for (size_t i = 0; i < want.size(); ++i) CHECK(tm.Qpad[(size_t)m * Dp2 * Dp2 + i] == want[i]);
  }
}

int main() {
  check_dim(3, 12);
  check_dim(12, 0);
  check_dim(47, 0);

  // the list of instantiations, at its edges
  curD = 0;
  const int has[] = {12, 16, 20, 24, 25, 30, 32, 40, 46};
  for (int D = 1; D <= 64; ++D) {
    bool h = false;
    int next = 0;
    for (int d : has) {
      h = h || d == D;
      if (!next && d > D) next = d;
    }
    CHECK(traj_blk_has(D) == h);
    CHECK(traj_blk_padded_dim(D) == (h ? 0 : next));
  }

  // A = 0, Syy = diag(1, .., 1, -1) in mixture 2: Q_2 = inv(Syy) is indefinite -> the model converts, without c_m
  {
    curD = 3;
    const int D2 = 6, M = 2;
    const size_t nn = (size_t)D2 * D2;
    Inputs in = make_inputs(D2, M, 99);
    for (size_t i = 0; i < nn; ++i) in.A[nn + i] = in.Sxy[nn + i] = in.Syy[nn + i] = 0.0;
    for (int r = 0; r < D2; ++r) in.Syy[nn + (size_t)r * D2 + r] = r + 1 < D2 ? 1.0 : -1.0;
    TrajModel tm;
    CHECK(traj_prepare_model(in.A, in.Sxy, in.Syy, in.mux, in.muy, D2, M, tm) == VCMI_OK);
    CHECK(!tm.em_pd);
    CHECK(tm.Q[nn + nn - 1] == -1.0);
    // a singular conditional covariance is refused
    for (int r = 0; r < D2; ++r) in.Syy[nn + (size_t)r * D2 + r] = 0.0;
    CHECK(traj_prepare_model(in.A, in.Sxy, in.Syy, in.mux, in.muy, D2, M, tm) == VCMI_ERR_NOT_PD);
  }

  if (bad) {
    printf("traj_prepare_check: %d checks failed\n", bad);
    return 1;
  }
  printf("traj_prepare_check: ok\n");
  return 0;
}
