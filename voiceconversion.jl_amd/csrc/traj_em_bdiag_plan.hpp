// traj_em_bdiag_plan.hpp -- the launch rule of traj_em_bd_kernel (traj_em_bdiag.hip): frames per workgroup, its LDS, the tile
// job list of a call and the scratch arithmetic of EM re-estimation over a cross-diagonal trajectory converter.  HOST
// arithmetic only, no HIP: tests/c/traj_em_bdiag_plan_check.cpp compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vcmi {

static constexpr int kEmBdThreads = 512;                   // eight waves, lane = frame
static constexpr size_t kEmBdLdsBudget = 160 * 1024;       // the LDS of a CU
static constexpr int kEmBdMaxDP = 128, kEmBdMaxM = 256;    // every model vcmi_bdmap_create accepts (gmmmap_bdiag_prepare.hpp)

// One workgroup: frames [t0, t0 + FB) of utterance `utt` (its position in the call's sorted descriptor list).
struct EmBdJob {
  int32_t utt, t0;
};

// LDS of a workgroup in bytes: x and Y = W y of the tile [DP][FB + 1] each (the results of phase 3 take their place), one
// (mixture, frame) table [M][FB] that holds l, then the joint log-density, then gamma, and the NP partial results of a frame.
inline size_t em_bd_lds_bytes(int DP, int M, int FB) {
  return ((size_t)2 * DP * (FB + 1) + (size_t)M * FB + kEmBdThreads) * sizeof(double);
}

// Frames per workgroup: 64 where the tiles fit the budget, else 32 (which fit for every model: static_assert below).
inline int em_bd_frames(int DP, int M) { return em_bd_lds_bytes(DP, M, 64) <= kEmBdLdsBudget ? 64 : 32; }
static_assert(((size_t)2 * kEmBdMaxDP * 33 + (size_t)kEmBdMaxM * 32 + kEmBdThreads) * sizeof(double) <= kEmBdLdsBudget,
              "the 32-frame tiles of the largest model fit a CU");

// The tile jobs of a call over utterances of T[0 .. n) frames (in the order of the descriptors): every frame of every utterance
// in exactly one job, no job across utterances, an empty utterance in none.
inline void em_bd_jobs(const int32_t *T, int n, int FB, std::vector<EmBdJob> *jobs) {
  jobs->clear();
  for (int u = 0; u < n; ++u)
    for (int64_t t0 = 0; t0 < T[u]; t0 += FB) jobs->push_back(EmBdJob{(int32_t)u, (int32_t)t0});
}
inline int64_t em_bd_job_count(const int32_t *T, int n, int FB) {
  int64_t c = 0;
  for (int u = 0; u < n; ++u) c += ((int64_t)T[u] + FB - 1) / FB;
  return c;
}

// The solver reads the low 32 bits of the identity index f + 1 over the call's packed frames.
inline bool em_bd_frames_ok(int64_t nframes) { return nframes >= 0 && nframes <= (int64_t)INT32_MAX - 1; }

// Scratch of a call in elements: the blended precisions qbar (doubles), lse (doubles), the identity index (int64), L (doubles).
inline int64_t em_bd_qbar_doubles(int64_t nframes, int D2) { return nframes * D2; }
inline int64_t em_bd_lse_doubles(int64_t nframes) { return nframes; }
inline int64_t em_bd_index_words(int64_t nframes) { return nframes; }
inline int64_t em_bd_L_doubles(int iters, int n) { return (int64_t)iters * n; }
inline int64_t em_bd_scratch_bytes(int64_t nframes, int D2, int iters, int n) {
  return 8 * (em_bd_qbar_doubles(nframes, D2) + em_bd_lse_doubles(nframes) + em_bd_index_words(nframes) + em_bd_L_doubles(iters, n));
}

}  // namespace vcmi
