// traj_gvd_plan_check.cpp -- the launch rule of traj_gvd_kernel and the workspace arithmetic of a GV call over diagonal conditional
// precisions (csrc/traj_band_plan.hpp: host arithmetic, no HIP) on the CPU.  Asserts the rule's invariants over every static
// dimension the kernel takes and utterance lengths up to 2^31 - 1, exact values at the shapes DESIGN 3.5-DIAG names, and prints
// "rule D T resident lds_bytes" lines, which tests/test_traj_gvd_plan_host.py compares with the rule as Python restates it
// (tests/gv_diag_restatement.py: gvd_resident).  Built by that test with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdint>

#include "../../voiceconversion.jl_amd/csrc/traj_band_plan.hpp"

using namespace vcmi;

static int bad = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      if (++bad <= 20) printf("traj_gvd_plan_check: %s (line %d)\n", #cond, __LINE__);     \
    }                                                                                      \
  } while (0)

int main() {
  static const int64_t Ts[] = {2, 3, 4, 5, 16, 17, 33, 50, 64, 65, 70, 100, 300, 323, 324, 403, 404, 538, 539, 807, 808, 2000, 29313,
                               1000000, 2147483647};
  for (int D = 1; D <= kGvdThreads; ++D) {
    int prev = kGvdArrays;
    for (int64_t T : Ts) {
      const int r = gvd_resident(D, T);
      const size_t lds = gvd_lds_bytes(D, T);
      CHECK(r == 0 || (r >= 2 && r <= kGvdArrays));
      CHECK(lds <= kGvdLdsLimit);                                  // what the launch asks for always fits
      CHECK(lds == gvd_fixed_lds_bytes(D) + (size_t)r * (size_t)T * D * 8);
      CHECK(r <= prev);                                            // a longer utterance never keeps more
      // the rule keeps as much as fits: one more array would not
      if (r < kGvdArrays && r >= 2) CHECK(gvd_fixed_lds_bytes(D) + (size_t)(r + 1) * (size_t)T * D * 8 > kGvdLdsLimit);
      if (r == 0) CHECK(gvd_fixed_lds_bytes(D) + 2 * (size_t)T * D * 8 > kGvdLdsLimit);
      prev = r;
      if (D == 1 || D == 4 || D == 12 || D == 33 || D == 40 || D == 59 || D == 64 || D == 160 || D == 512)
        printf("rule %d %lld %d %zu\n", D, (long long)T, r, lds);
    }
  }
  // the shapes DESIGN names: vc's chunks at the headline dimension keep four arrays, the long utterances are streamed, the edges
  // of the forms at D = 12
  CHECK(gvd_resident(40, 100) == 4 && gvd_resident(40, 2000) == 0 && gvd_resident(59, 2000) == 0 && gvd_resident(40, 300) == 0);
  CHECK(gvd_resident(12, 323) == 5 && gvd_resident(12, 324) == 4 && gvd_resident(12, 403) == 4 && gvd_resident(12, 404) == 3);
  CHECK(gvd_resident(12, 538) == 3 && gvd_resident(12, 539) == 2 && gvd_resident(12, 807) == 2 && gvd_resident(12, 808) == 0);
  CHECK(gvd_resident(40, 0) == 0 && gvd_lds_bytes(40, 0) == gvd_fixed_lds_bytes(40));
  // workspace: the solver's (nframes,D) alone, five of them with GV; no overflow at 2^31 frames of the widest dimension
  CHECK(gvd_ws_doubles(1000, 40, false) == 40000 && gvd_ws_doubles(1000, 40, true) == 200000 && gvd_ws_doubles(0, 40, true) == 0);
  CHECK(gvd_ws_doubles((int64_t)1 << 31, 512, true) == ((int64_t)5 << 40));
  if (bad) {
    printf("traj_gvd_plan_check: %d failures\n", bad);
    return 1;
  }
  printf("traj_gvd_plan_check: ok\n");
  return 0;
}
