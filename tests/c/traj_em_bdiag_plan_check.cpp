// traj_em_bdiag_plan_check.cpp -- the launch rule of traj_em_bd_kernel and the scratch arithmetic of EM re-estimation over a
// cross-diagonal trajectory converter (csrc/traj_em_bdiag_plan.hpp: host arithmetic, no HIP) on the CPU.  Asserts for every padded
// feature dimension up to 128 and every mixture count up to 256 that the tiles fit the LDS of a CU and that 64 frames are taken
// exactly where they fit; for a grid of batches that every frame of every utterance lies in exactly one job and no job crosses
// an utterance; the frame limit of the identity index; the scratch sizes.  Prints "rule DP M FB lds_bytes" lines at the shapes
// DESIGN 3.4-BDIAG-EM names.  Built by tests/test_traj_em_bdiag_host.py with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../voiceconversion.jl_amd/csrc/traj_em_bdiag_plan.hpp"

using namespace vcmi;

static int bad = 0;
#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      if (++bad <= 20) printf("traj_em_bdiag_plan_check: %s (line %d)\n", #cond, __LINE__);  \
    }                                                                                        \
  } while (0)

static void check_jobs(const std::vector<int32_t> &T, int FB) {
  std::vector<EmBdJob> jobs;
  em_bd_jobs(T.data(), (int)T.size(), FB, &jobs);
  CHECK((int64_t)jobs.size() == em_bd_job_count(T.data(), (int)T.size(), FB));
  std::vector<std::vector<int>> seen(T.size());
  for (size_t u = 0; u < T.size(); ++u) seen[u].assign((size_t)T[u], 0);
  for (const EmBdJob &j : jobs) {
    CHECK(j.utt >= 0 && (size_t)j.utt < T.size());
    if (j.utt < 0 || (size_t)j.utt >= T.size()) continue;
    CHECK(j.t0 >= 0 && j.t0 < T[(size_t)j.utt] && j.t0 % FB == 0);           // never empty, never across the utterance's end
    for (int t = j.t0; t < j.t0 + FB && t < T[(size_t)j.utt]; ++t) seen[(size_t)j.utt][(size_t)t] += 1;
  }
  for (size_t u = 0; u < T.size(); ++u)
    for (int c : seen[u]) CHECK(c == 1);
  for (size_t k = 1; k < jobs.size(); ++k)                                       // in the order of the descriptors, frames ascending
    CHECK(jobs[k].utt > jobs[k - 1].utt || (jobs[k].utt == jobs[k - 1].utt && jobs[k].t0 == jobs[k - 1].t0 + FB));
}

int main() {
  for (int DP = 4; DP <= kEmBdMaxDP; DP += 4)
    for (int M = 1; M <= kEmBdMaxM; ++M) {
      const int FB = em_bd_frames(DP, M);
      CHECK(FB == 64 || FB == 32);
      CHECK(em_bd_lds_bytes(DP, M, FB) <= kEmBdLdsBudget);
      CHECK((FB == 64) == (em_bd_lds_bytes(DP, M, 64) <= kEmBdLdsBudget));       // 64 frames wherever they fit
      CHECK(em_bd_lds_bytes(DP, M, FB) == ((size_t)2 * DP * (FB + 1) + (size_t)M * FB + 512) * 8);
      CHECK(kEmBdThreads % FB == 0 && 64 % FB == 0);
      if ((DP == 80 || DP == 120 || DP == 128) && (M == 8 || M == 64 || M == 128 || M == 256))
        printf("rule %d %d %d %zu\n", DP, M, FB, em_bd_lds_bytes(DP, M, FB));
    }
  CHECK(em_bd_frames(80, 64) == 64 && em_bd_frames(120, 64) == 64 && em_bd_frames(128, 64) == 32 && em_bd_frames(8, 256) == 64);
  CHECK(em_bd_frames(128, 256) == 32);
  for (int FB : {32, 64}) {
    check_jobs({}, FB);
    check_jobs({0}, FB);
    check_jobs({1}, FB);
    check_jobs({63, 64, 65, 129, 1}, FB);
    check_jobs({300, 0, 130, 0, 0, 31, 32, 33}, FB);
    check_jobs({2000, 2000, 100, 7}, FB);
    std::vector<int32_t> many(5120, 100);
    check_jobs(many, FB);
    check_jobs({INT32_MAX / 1024}, FB);
  }
  const int32_t big[1] = {INT32_MAX};
  CHECK(em_bd_job_count(big, 1, 32) == ((int64_t)INT32_MAX + 31) / 32);
  // the identity index f + 1 must fit the 32 bits the solver reads
  CHECK(em_bd_frames_ok(0) && em_bd_frames_ok((int64_t)INT32_MAX - 1) && !em_bd_frames_ok((int64_t)INT32_MAX) && !em_bd_frames_ok(-1));
  // scratch: qbar (nframes, 2D), lse, the index, L (iterations, utterances); no overflow at the frame limit and 2D = 128
  CHECK(em_bd_qbar_doubles(512000, 80) == 40960000 && em_bd_lse_doubles(512000) == 512000 && em_bd_index_words(512000) == 512000);
  CHECK(em_bd_L_doubles(2, 256) == 512 && em_bd_L_doubles(0, 256) == 0);
  CHECK(em_bd_scratch_bytes(512000, 80, 2, 256) == 8 * (int64_t)(40960000 + 512000 + 512000 + 512));
  CHECK(em_bd_qbar_doubles((int64_t)INT32_MAX - 1, 128) == ((int64_t)INT32_MAX - 1) * 128);
  if (bad) {
    printf("traj_em_bdiag_plan_check: %d failures\n", bad);
    return 1;
  }
  printf("traj_em_bdiag_plan_check: ok\n");
  return 0;
}
