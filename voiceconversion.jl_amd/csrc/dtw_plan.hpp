// dtw_plan.hpp -- the host planning of the fused DTW path (dtw_fused.hip): from the pairs of a call, the job list its forward
// kernel runs -- row strips, packed groups, column segments, the flags that order them -- and every workspace offset.  No HIP
// call and no device type: tests/c/dtw_plan_check.cpp checks it without a device.  What it must guarantee above all: a job
// waits only on flags that a job EARLIER in the list signals, which is what keeps dtw_fused_persistent_kernel from deadlock.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vcmi {

// One pair of a DTW call, as the kernels of every path read it (device image).
struct DtwPair {
  int64_t tmpl_off;     // template (D,S) at feats + tmpl_off
  int64_t seq_off;      // sequence (D,T) at feats + seq_off
  int64_t *path;        // (T) 1-based, may be null when only newtgt is wanted
  double *cost;         // (S,T+1) or null
  int64_t *bp;          // (S,T+1) or null
  double *newtgt;       // (D,S) or null: align() output
  unsigned char *codes; // (S,T) bytes in HBM, used only when the step codes do not fit in LDS
  int64_t obs_off;      // (S,T) observation costs at obs_ws + obs_off (fast path workspace)
  int64_t spad_off;     // offset of the zero-padded sequence copy (fast path, D != DMAX)
  int64_t tpad_off;     // offset of the zero-padded template copy (same workspace)
  int64_t fcodes_off;   // fused path: this pair's packed step codes, [ceil(T/16)][Se] dwords at fcodes_ws + fcodes_off
  int64_t clast_off;    // fused path: last cost column (S doubles) at clast_ws + clast_off
  int64_t path32_off;   // fused path: the pair's 0-based path (T ints) at path32_ws + path32_off
  int32_t S, T;
};

// One workgroup of the fused kernel: rows [row0, row0 + nrows) of a pair ("row strip").  Row r of column t+1 depends
// only on rows r, r-1, r-2 of column t (src/dtw.jl:107-121 with fstep = 0), so a strip needs nothing from the rows above
// it: a template longer than one workgroup's 512 rows is processed bottom strip first, each strip leaving the costs of
// its top two rows (per column) for the next one.
struct DtwStrip {
  int32_t pair, row0, nrows;
  int32_t flag_in, flag_out;     // indices into the flag array (-1: none): wait for / signal the neighbouring strip
  int64_t bnd_in, bnd_out;       // offsets (doubles) into bnd_ws of the (T,2) boundary arrays, -1: none
  // column segment [col0, col0 + ncol) of the pair (a multiple of 16 columns unless it is the last): a strip's columns are
  // cut into segments that run as separate jobs, so that the ~equal jobs of a batch do not come in a whole number per
  // slot (see dtw_run_fused); flag_prev: the job of the same strip's previous segment (-1: first segment)
  int32_t col0, ncol, flag_prev, packed;     // packed: member of a packed group of four one-wave strips
};

static constexpr int kFusedRows = 512;        // rows per strip (4 waves x 64 lanes x 2 rows)

struct DtwFusedPlan {
  std::vector<DtwStrip> strips;    // the descriptors of all jobs, in job order
  std::vector<int> job_first;      // first descriptor of every job (one descriptor, or the four of a packed group)
  int nflags = 0;                  // flag indices handed out (flag_in / flag_out / flag_prev are below it)
  int nseg = 1;                    // column segments per strip
  bool any_align = false;          // some pair wants newtgt
  // workspace sizes: packed step codes (dwords), last cost columns, strip boundaries, padded features (doubles), paths (ints)
  size_t ncodes = 0, nclast = 0, nbnd = 0, padn = 0, npath = 0;
};

// Sorts `pairs` largest first, sets their fcodes_off / clast_off / path32_off / spad_off / tpad_off and returns the job list.
// row_len: doubles per frame of the padded feature copies (dtw_fused_row); slots: workgroups the device holds at once;
// segments_allowed / two_segments_max / whole_first: the test hooks kDbgDtwNoSegments (negated), kDbgDtwTwoSegments and
// kDbgDtwWholeFirst, which the caller reads.
DtwFusedPlan dtw_fused_plan(std::vector<DtwPair> &pairs, int row_len, int slots, bool segments_allowed, bool two_segments_max,
                            bool whole_first);

}  // namespace vcmi
