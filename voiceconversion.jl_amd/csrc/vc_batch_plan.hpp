// vc_batch_plan.hpp -- the host planning of vc_batch (vc_batch.hip): from the utterance lengths of a call, the verdict on the
// call and every list its kernels index.  No HIP call and no device type: tests/c/vc_batch_plan_check.cpp checks it without a
// device.
//
// The rule (include/vcmi.h, vcmi_vc_traj_batch): utterance u of the batch converts as vc(c_u, fm_u) would on a fresh converter
// c_u with length(c_u) = L.  So every utterance is cut into chunks [kL+1, min((k+1)L, T_u)] of its OWN frames, the deltas and the
// post-filter's statistics are per utterance, and the frames of all utterances lie back to back in one packed matrix.
#pragma once
#include <cstdint>
#include <vector>

namespace vcmi {

static constexpr int kVcbTileFrames = 128;    // frames of one (utterance, tile) item of the pre and post kernels
static constexpr int kVcbStatFrames = 2048;   // frames of one statistics item: kVsChunk of postf.hip, whose order it reproduces

struct VcbUtt {          // one utterance as the kernels see it (device image: four 64-bit words)
  int64_t in_off;        // doubles from the input base to its (rows_in, T) matrix
  int64_t out_off;       // doubles from the output base to its (rows_out, T) result
  int64_t frame0;        // its first frame in the packed matrices
  int64_t T;
};
struct VcbItem {         // a work item of any of the three kernels (device image: two 32-bit words)
  int32_t utt;
  int32_t first;         // pre / post: first frame of the tile in the utterance; statistics: index of the 2048-frame chunk
};
struct VcbChunk {        // one fvconvert of the trajectory solver
  int32_t utt;
  int32_t T;             // its length, 1 .. L
  int64_t frame0;        // its first frame in the packed matrices
};

struct VcBatchPlan {
  int status = 0;                    // VCMI_OK, VCMI_ERR_DIM or VCMI_ERR_ARG (include/vcmi.h); the lists are empty unless VCMI_OK
  const char *why = "";              // the refusal, for vcmi_last_error
  int64_t nframes = 0;               // sum of T
  std::vector<VcbUtt> utts;          // n
  std::vector<VcbItem> tiles;        // sum over u of ceil(T_u / kVcbTileFrames), utterances in order
  std::vector<VcbItem> stat_items;   // with a filter: sum over u of ceil(T_u / kVcbStatFrames), utterances in order
  std::vector<int64_t> stat_first;   // with a filter: n + 1, utterance u owns the items [stat_first[u], stat_first[u+1])
  std::vector<VcbChunk> chunks;      // chunked converters: sum over u of ceil(T_u / L), utterances in order
};

// n utterances of T[u] frames; chunked: a trajectory converter with length L (a frame-by-frame converter ignores L);
// rows_in / rows_out: rows of an utterance's input and result, which lie dense at in_off[u] / out_off[u] -- or, where the
// pointer is NULL, back to back (offset rows * frame0).  Refusals, in this order: n < 0 or a NULL T with n > 0 or a negative
// T[u]: VCMI_ERR_ARG; chunked and L < 1: VCMI_ERR_ARG; a length or chunk count beyond int32: VCMI_ERR_DIM; a filter with some
// T[u] == 1: VCMI_ERR_DIM; a GV converter with a one-frame chunk (T[u] mod L == 1): VCMI_ERR_DIM.
VcBatchPlan vc_batch_plan(int64_t n, const int64_t *T, bool chunked, int64_t L, int rows_in, int rows_out, bool has_filter,
                          bool is_gv, const int64_t *in_off = nullptr, const int64_t *out_off = nullptr);

}  // namespace vcmi
