// estep_plan.hpp -- the launch plan of one diagonal E-step (estep.hip): from the call's shape, the device's CU count, the
// thread's path choice and the test hooks, WHICH kernels run and with what -- the route, the grid of every launch, the rows of
// every fixed-order reduction, the element count of every scratch reservation.  No HIP call and no device type:
// tests/c/estep_plan_check.cpp checks it without a device.  The launchers of estep.hip decide nothing themselves; the one
// thing they may still do is demote a wanted hard-assignment chain when the soft frames' matrix cannot be allocated.
#pragma once
#include <cstddef>
#include <cstdint>

#include "estep_cfg.hpp"

namespace vcmi {

enum EstepRoute {
  kRouteGeneric,      // any Dj, M: estep_gamma_kernel / estep_stats_kernel in chunks of kChunk frames
  kRoutePadOdd,       // odd Dj <= 159: chunks of kPadChunk frames padded to Dj + 1, each planned again as kRouteMfma / kRouteGroups
  kRouteGroups,       // even Dj <= 160, M > 128: groups of 128 mixtures, chunks of kGroupsChunk frames
  kRouteMfma          // even Dj <= 160, M <= 128: estep_mfma_launch
};
enum EstepBody {
  kBodySmall1,        // estep_small_kernel<DJ, 1>: M <= 16
  kBodySmall2,        // estep_small_kernel<DJ, 2>: M <= 32
  kBodyOne,           // estep_mfma_kernel<DJ, 0, share>
  kBodyWave,          // estep_wave_kernel<DJ>: the test hook, M > 64
  kBodySplit          // estep_mfma_kernel<DJ, 1, share> + <DJ, 2, share> per chunk of kSplitChunk frames: DJ > 80
};

struct EstepPlanInput {
  int64_t N = 0;               // frames, > 0
  int Dj = 0, M = 0;           // joint dimension, mixtures: >= 1
  int cus = 0;                 // compute units of the device (unused by kRouteGeneric)
  int path = 0;                // VCMI_ESTEP_AUTO / _HARD / _SOFT of the calling thread
  bool generic = false, no_small = false, no_hard = false, wave_kernel = false;      // kDbgEstepGeneric, ...NoSmall, ...NoHard, ...WaveKernel
  bool device_block = false;   // the parameters are a device block (estep_device_block), not three host arrays
};

// A route that runs in chunks of frames: `count` chunks of `len` frames, the last one of `last` (1 <= last <= len).  What
// depends on a chunk's frames comes in pairs below: [0] a chunk of `len` frames, [1] the last chunk.
struct EstepChunks {
  int64_t len = 0, count = 0, last = 0;
};

struct EstepPlan {
  EstepRoute route = kRouteGeneric;
  // a device block whose route needs the parameters on the host (every route but kRouteMfma pads, regroups or transposes them)
  bool copy_down = false;
  int64_t plen = 0;            // vcmi_estep_stats_len(Dj, M)
  EstepChunks chunks;          // (kRouteMfma: the body kBodySplit; one chunk of N frames otherwise)
  int reduce_grid = 0;         // estep_reduce_kernel over rows of plen doubles

  // ---- scratch reservations (elements of the buffer's type; 0: not reserved by this route) ----
  size_t n_part = 0;           // partial statistics: the maximum over the launches of the chain
  size_t n_G = 0, n_LSE = 0;   // responsibilities and log-sum-exps through HBM (generic, groups, kBodySplit)
  size_t n_mu = 0, n_cst = 0;  // generic: mu / iv (M Dj each), the constants (M)
  size_t n_Xpad = 0, n_statsp = 0;                                     // pad-odd: a padded chunk, its statistics
  size_t n_raw = 0, n_Wpack = 0, n_cinit = 0, n_refiv = 0, n_refc = 0; // MFMA operands (n_raw: one staging slot)
  size_t n_Xsoft = 0, n_W16 = 0, n_probe = 0, n_ctl = 0, n_hkeys = 0, n_hpart = 0, n_hllm = 0;      // the hard chain

  // ---- kRouteGeneric ----
  int gamma_grid[2] = {0, 0}, nseg[2] = {0, 0};      // estep_gamma_kernel; segments = grid.x of estep_stats_kernel = rows of the reduce
  int stats_grid_y = 0;
  size_t gamma_lds = 0;        // bytes (the launcher refuses more than 150 KB)

  // ---- kRoutePadOdd ----
  int djp = 0;                 // Dj + 1
  int64_t plen_p = 0;          // vcmi_estep_stats_len(djp, M)
  int pad_grid[2] = {0, 0}, unpad_grid = 0;

  // ---- kRouteGroups and kRouteMfma ----
  int DJ = 0;                  // estep_mfma_dj(Dj)
  int prep_grid = 0;           // estep_prep_kernel (one launch per group)
  // kRouteGroups: ng groups, the last of Mg_last mixtures; PHASE 3 / PHASE 2 grid per chunk (= rows of the group's reduce);
  // estep_group_reduce_kernel for [0] a group of 128, [1] the last group
  int ng = 0, Mg_last = 0, group_grid[2] = {0, 0}, group_reduce_grid[2] = {0, 0};

  // ---- kRouteMfma ----
  int mtp = 0, wpt = 0;        // mixture tiles of 16 rounded up to a power of two; waves per tile = 8 / mtp
  bool share = false;          // mtp < 8: the SHARE instantiations
  EstepBody body = kBodyOne;   // what runs over the call's frames (without the hard chain, or when it was demoted)
  size_t body_lds = 0;         // dynamic LDS bytes of the body's kernel
  // the body's grid and the rows of its reduce; kBodySplit: per chunk ([0] / [1] as above), otherwise [0] over all N frames
  int body_grid[2] = {0, 0}, body_rows[2] = {0, 0};
  // The hard-assignment chain (DJ <= 80): wanted?  Its FP64 launches are soft_body (never kBodyWave): over the gathered soft
  // frames, their number on the device (a grid that covers the CUs), then -- sample: the path is decided on the device --
  // over all N frames.
  bool hard = false, sample = false;
  EstepBody soft_body = kBodyOne;
  size_t soft_lds = 0;
  int gathered_grid = 0, gathered_rows = 0, allsoft_grid = 0, allsoft_rows = 0;
  int MT = 0, MK = 0;          // mixture tiles of 16; keys (M + 1: the last is "soft")
  int64_t nchunks = 0, nsample = 0, cstride = 0;     // chunks of kHardChunk frames; sampled chunks and their stride
  int64_t npmax = 0, prow = 0; // pieces of kHardPiece hard frames (upper bound) and doubles per piece
  int hprep_grid = 0, sample_grid = 0, key_grid = 0, scan_grid = 0, scatter_grid = 0, hstats_grid = 0, hreduce_grid = 0, gather_grid = 0;
  size_t key_lds = 0, scatter_lds = 0;
};

EstepPlan estep_plan(const EstepPlanInput &in);

}  // namespace vcmi
