// vc_batch_plan.cpp -- see vc_batch_plan.hpp.  Host arithmetic only.
#include "vc_batch_plan.hpp"

#include <algorithm>

#include "../../include/vcmi.h"

namespace vcmi {

static VcBatchPlan refuse(int status, const char *why) {
  VcBatchPlan p;
  p.status = status;
  p.why = why;
  return p;
}

VcBatchPlan vc_batch_plan(int64_t n, const int64_t *T, bool chunked, int64_t L, int rows_in, int rows_out, bool has_filter,
                          bool is_gv, const int64_t *in_off, const int64_t *out_off) {
  if (n < 0 || (n > 0 && !T)) return refuse(VCMI_ERR_ARG, "vc_batch: bad argument");
  for (int64_t u = 0; u < n; ++u)
    if (T[u] < 0) return refuse(VCMI_ERR_ARG, "vc_batch: negative utterance length");
  if (chunked && L < 1) return refuse(VCMI_ERR_ARG, "vc_batch: length(t) must be positive");
  if (n > INT32_MAX) return refuse(VCMI_ERR_DIM, "vc_batch: too many utterances");
  int64_t nchunks = 0, ntiles = 0, nstat = 0;
  for (int64_t u = 0; u < n; ++u) {
    if (T[u] > INT32_MAX) return refuse(VCMI_ERR_DIM, "vc_batch: bad utterance length");
    if (has_filter && T[u] == 1) return refuse(VCMI_ERR_DIM, "vc_batch: the variance of a one-frame matrix is undefined");
    if (chunked && is_gv && (L == 1 ? T[u] > 0 : T[u] % L == 1))    // (L = 1: every chunk has one frame)
      return refuse(VCMI_ERR_DIM, "vc_batch: the variance of a one-frame trajectory is undefined");
    if (chunked) nchunks += (T[u] + L - 1) / L;
    ntiles += (T[u] + kVcbTileFrames - 1) / kVcbTileFrames;
    nstat += (T[u] + kVcbStatFrames - 1) / kVcbStatFrames;
  }
  if (nchunks > INT32_MAX) return refuse(VCMI_ERR_DIM, "vc_batch: too many chunks");
  VcBatchPlan p;
  p.utts.resize((size_t)n);
  p.tiles.reserve((size_t)ntiles);
  if (chunked) p.chunks.reserve((size_t)nchunks);
  if (has_filter) {
    p.stat_items.reserve((size_t)nstat);
    p.stat_first.assign((size_t)n + 1, 0);
  }
  int64_t f0 = 0;
  for (int64_t u = 0; u < n; ++u) {
    const int64_t Tu = T[u];
    p.utts[(size_t)u] = VcbUtt{in_off ? in_off[u] : f0 * rows_in, out_off ? out_off[u] : f0 * rows_out, f0, Tu};
    for (int64_t t = 0; t < Tu; t += kVcbTileFrames) p.tiles.push_back(VcbItem{(int32_t)u, (int32_t)t});
    if (chunked)
      for (int64_t t = 0; t < Tu; t += L) p.chunks.push_back(VcbChunk{(int32_t)u, (int32_t)std::min<int64_t>(L, Tu - t), f0 + t});
    if (has_filter) {
      for (int64_t c = 0; c * kVcbStatFrames < Tu; ++c) p.stat_items.push_back(VcbItem{(int32_t)u, (int32_t)c});
      p.stat_first[(size_t)u + 1] = (int64_t)p.stat_items.size();
    }
    f0 += Tu;
  }
  p.nframes = f0;
  return p;
}

}  // namespace vcmi
