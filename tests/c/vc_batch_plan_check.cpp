// vc_batch_plan_check.cpp -- exact facts about the host planning of vc_batch (csrc/vc_batch_plan.cpp): chunk counts and bounds,
// work-list lengths, offsets and every refusal verdict, at T = [0, 1, 2, L-1, L, L+1, 2L+1, 2048, 2049] and L in {1, 20}.
// Stand-alone (no device, no HIP); tests/test_vc_batch_host.py builds it with ASan + UBSan and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/vcmi.h"
#include "../../voiceconversion.jl_amd/csrc/vc_batch_plan.hpp"

using namespace vcmi;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// every list of an accepted plan against its definition, element by element
static void check_lists(const VcBatchPlan &p, const std::vector<int64_t> &T, bool chunked, int64_t L, int rows_in, int rows_out,
                        bool has_filter) {
  const size_t n = T.size();
  CHECK(p.status == VCMI_OK);
  CHECK(p.utts.size() == n);
  int64_t f0 = 0;
  size_t tile = 0, chunk = 0, item = 0;
  for (size_t u = 0; u < n; ++u) {
    CHECK(p.utts[u].frame0 == f0 && p.utts[u].T == T[u]);
    CHECK(p.utts[u].in_off == f0 * rows_in && p.utts[u].out_off == f0 * rows_out);
    for (int64_t t = 0; t < T[u]; t += kVcbTileFrames, ++tile) {
      CHECK(tile < p.tiles.size());
      if (tile < p.tiles.size()) CHECK(p.tiles[tile].utt == (int32_t)u && p.tiles[tile].first == t);
    }
    if (chunked) {
      // chunks [kL+1, min((k+1)L, T)] of this utterance's own frames: all of length L but the last, which has the rest
      const int64_t nch = cdiv(T[u], L);
      for (int64_t k = 0; k < nch; ++k, ++chunk) {
        CHECK(chunk < p.chunks.size());
        if (chunk >= p.chunks.size()) continue;
        const VcbChunk &c = p.chunks[chunk];
        CHECK(c.utt == (int32_t)u && c.frame0 == f0 + k * L);
        CHECK(c.T == (k + 1 < nch ? L : T[u] - k * L) && c.T >= 1 && c.T <= L);
      }
    }
    if (has_filter) {
      CHECK(p.stat_first.size() == n + 1 && p.stat_first[u] == (int64_t)item);
      for (int64_t c = 0; c < cdiv(T[u], kVcbStatFrames); ++c, ++item) {
        CHECK(item < p.stat_items.size());
        if (item < p.stat_items.size()) CHECK(p.stat_items[item].utt == (int32_t)u && p.stat_items[item].first == c);
      }
    }
    f0 += T[u];
  }
  CHECK(p.nframes == f0);
  CHECK(p.tiles.size() == tile);
  CHECK(p.chunks.size() == (chunked ? chunk : 0));
  CHECK(p.stat_items.size() == (has_filter ? item : 0));
  if (has_filter) CHECK(p.stat_first.size() == n + 1 && p.stat_first[n] == (int64_t)item);
  else CHECK(p.stat_first.empty());
}

static void check_refused(const VcBatchPlan &p, int status) {
  CHECK(p.status == status && p.why && p.why[0]);
  CHECK(p.utts.empty() && p.tiles.empty() && p.chunks.empty() && p.stat_items.empty() && p.stat_first.empty() && p.nframes == 0);
}

static std::vector<int64_t> without(std::vector<int64_t> T, bool (*drop)(int64_t, int64_t), int64_t L) {
  std::vector<int64_t> r;
  for (int64_t t : T)
    if (!drop(t, L)) r.push_back(t);
  return r;
}

int main() {
  const int D = 12;
  for (int64_t L : {(int64_t)1, (int64_t)20}) {
    const std::vector<int64_t> T = {0, 1, 2, L - 1, L, L + 1, 2 * L + 1, 2048, 2049};
    const int64_t n = (int64_t)T.size();
    // plain trajectory converter, static and (2D+1) input, no filter: everything is accepted
    for (int rows_in : {D + 1, 2 * D + 1}) {
      const VcBatchPlan p = vc_batch_plan(n, T.data(), true, L, rows_in, D + 1, false, false);
      check_lists(p, T, true, L, rows_in, D + 1, false);
    }
    // exact counts at L = 20: chunks 0 1 1 1 1 2 3 103 103, tiles 0 1 1 1 1 1 1 16 17, statistics items 0 1 1 1 1 1 1 1 2
    if (L == 20) {
      const VcBatchPlan p = vc_batch_plan(n, T.data(), true, L, D + 1, D + 1, false, false);
      CHECK(p.chunks.size() == 215 && p.tiles.size() == 39 && p.nframes == 0 + 1 + 2 + 19 + 20 + 21 + 41 + 2048 + 2049);
      CHECK(p.chunks[4].utt == 5 && p.chunks[4].T == 20 && p.chunks[5].utt == 5 && p.chunks[5].T == 1);       // T = 21: 20 + 1
      CHECK(p.chunks[8].utt == 6 && p.chunks[8].T == 1 && p.chunks[8].frame0 == 63 + 40);                      // T = 41: 20 + 20 + 1
      CHECK(p.chunks.back().utt == 8 && p.chunks.back().T == 9);                                              // 2049 = 102 * 20 + 9
      CHECK(p.utts[8].frame0 == 2152 && p.utts[8].in_off == 2152 * (D + 1));
    } else {
      const VcBatchPlan p = vc_batch_plan(n, T.data(), true, L, D + 1, D + 1, false, false);
      CHECK((int64_t)p.chunks.size() == p.nframes && p.nframes == 0 + 1 + 2 + 0 + 1 + 2 + 3 + 2048 + 2049);    // one frame each
      for (const VcbChunk &c : p.chunks) CHECK(c.T == 1);
    }
    // a filter refuses the one-frame utterances (T = 1, and L-1 / L / L+1 where they are 1) ...
    check_refused(vc_batch_plan(n, T.data(), true, L, D + 1, D + 1, true, false), VCMI_ERR_DIM);
    check_refused(vc_batch_plan(n, T.data(), false, 0, D + 1, D + 1, true, false), VCMI_ERR_DIM);
    // ... and accepts the batch without them; T = 0 stays in
    {
      const std::vector<int64_t> T2 = without(T, [](int64_t t, int64_t) { return t == 1; }, L);
      const VcBatchPlan p = vc_batch_plan((int64_t)T2.size(), T2.data(), true, L, 2 * D + 1, D + 1, true, false);
      check_lists(p, T2, true, L, 2 * D + 1, D + 1, true);
      CHECK(p.stat_items.size() >= 2 && p.stat_items.back().utt == (int32_t)T2.size() - 1 && p.stat_items.back().first == 1);
      const VcBatchPlan q = vc_batch_plan((int64_t)T2.size(), T2.data(), false, 0, D + 1, D + 1, true, false);   // frame by frame
      check_lists(q, T2, false, 0, D + 1, D + 1, true);
    }
    // a GV converter refuses a one-frame chunk in any utterance: T mod L == 1 (at L = 1 every non-empty utterance)
    check_refused(vc_batch_plan(n, T.data(), true, L, D + 1, D + 1, false, true), VCMI_ERR_DIM);
    {
      const std::vector<int64_t> T3 = without(T, [](int64_t t, int64_t l) { return t % l == 1 || (l == 1 && t > 0); }, L);
      const VcBatchPlan p = vc_batch_plan((int64_t)T3.size(), T3.data(), true, L, D + 1, D + 1, true, true);
      if (L == 1) CHECK(p.status == VCMI_OK && p.nframes == 0 && p.chunks.empty() && p.tiles.empty());    // only T = 0 is left
      check_lists(p, T3, true, L, D + 1, D + 1, true);
      for (const VcbChunk &c : p.chunks) CHECK(c.T >= 2);
      // each of the one-frame-chunk lengths alone is refused for GV and accepted without it
      for (int64_t t : T) {
        const bool bad = L == 1 ? t > 0 : t % L == 1;
        CHECK((vc_batch_plan(1, &t, true, L, D + 1, D + 1, false, true).status == VCMI_ERR_DIM) == bad);
        CHECK(vc_batch_plan(1, &t, true, L, D + 1, D + 1, false, false).status == VCMI_OK);
      }
    }
    // the caller's offsets are taken as they are (device-resident entries)
    {
      std::vector<int64_t> in_off(T.size()), out_off(T.size());
      for (size_t u = 0; u < T.size(); ++u) {
        in_off[u] = 1000 * (int64_t)(T.size() - u) - 7;
        out_off[u] = -3 + 5000 * (int64_t)u;
      }
      const VcBatchPlan p = vc_batch_plan(n, T.data(), true, L, D + 1, D + 1, false, false, in_off.data(), out_off.data());
      CHECK(p.status == VCMI_OK);
      for (size_t u = 0; u < T.size(); ++u) CHECK(p.utts[u].in_off == in_off[u] && p.utts[u].out_off == out_off[u]);
    }
  }
  // length(c) < 1, bad counts and lengths: VCMI_ERR_ARG; lengths beyond int32: VCMI_ERR_DIM; n = 0: an empty plan
  const int64_t one = 5, neg = -1, huge = (int64_t)INT32_MAX + 1;
  check_refused(vc_batch_plan(1, &one, true, 0, D + 1, D + 1, false, false), VCMI_ERR_ARG);
  check_refused(vc_batch_plan(1, &one, true, -3, D + 1, D + 1, true, true), VCMI_ERR_ARG);
  CHECK(vc_batch_plan(1, &one, false, 0, D + 1, D + 1, false, false).status == VCMI_OK);        // frame by frame: L is not read
  check_refused(vc_batch_plan(-1, &one, true, 20, D + 1, D + 1, false, false), VCMI_ERR_ARG);
  check_refused(vc_batch_plan(1, nullptr, true, 20, D + 1, D + 1, false, false), VCMI_ERR_ARG);
  check_refused(vc_batch_plan(1, &neg, true, 20, D + 1, D + 1, false, false), VCMI_ERR_ARG);
  check_refused(vc_batch_plan(1, &huge, true, 20, D + 1, D + 1, false, false), VCMI_ERR_DIM);
  {
    const VcBatchPlan p = vc_batch_plan(0, nullptr, true, 20, D + 1, D + 1, true, true);
    CHECK(p.status == VCMI_OK && p.nframes == 0 && p.utts.empty() && p.tiles.empty() && p.chunks.empty() && p.stat_items.empty());
    CHECK(p.stat_first.size() == 1 && p.stat_first[0] == 0);
  }
  if (failures) {
    std::printf("vc_batch_plan_check: %d FAILED\n", failures);
    return 1;
  }
  std::printf("vc_batch_plan_check: ok\n");
  return 0;
}
