// estep_plan_check.cpp -- exact facts about the launch plan of the diagonal E-step (csrc/estep_plan.cpp).  (a) A table of plans
// worked out by hand from the launch code the plan replaced, one per route, body and decision boundary, at 256 compute units;
// (b) properties over a sweep of shapes: every grid at least one workgroup, the partial-statistics buffer large enough for every
// reduction of the chain, the sample inside the chunks, the sort scratch and the piece count large enough for any assignment of
// frames to owners, nothing negative or beyond what an int argument holds.  Stand-alone (no device, no HIP);
// tests/test_estep_plan_host.py builds it with ASan + UBSan and runs it.  `--sequence N Dj M path flags cus` prints the kernel
// launches a plan stands for instead, in the form of a kernel trace (profiles/estep_plan/README.md compares the two).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>

#include "../../include/vcmi.h"
#include "../../voiceconversion.jl_amd/csrc/estep_plan.hpp"

using namespace vcmi;

static int failures = 0;
static char context[160] = "";
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      if (++failures <= 50) std::printf("FAILED %s:%d [%s]: %s\n", __FILE__, __LINE__, context, #cond); \
    }                                                                                \
  } while (0)
#define CHECK_EQ(a, b)                                                               \
  do {                                                                               \
    const long long a_ = (long long)(a), b_ = (long long)(b);                        \
    if (a_ != b_) {                                                                  \
      if (++failures <= 50) std::printf("FAILED %s:%d [%s]: %s = %lld, expected %lld\n", __FILE__, __LINE__, context, #a, a_, b_); \
    }                                                                                \
  } while (0)

enum Flag { kNone = 0, kGeneric = 1, kNoSmall = 2, kNoHard = 4, kWave = 8, kBlock = 16 };

static EstepPlan plan(int64_t N, int Dj, int M, int path = VCMI_ESTEP_AUTO, int flags = kNone, int cus = 256) {
  EstepPlanInput in;
  in.N = N;
  in.Dj = Dj;
  in.M = M;
  in.cus = cus;
  in.path = path;
  in.generic = flags & kGeneric;
  in.no_small = flags & kNoSmall;
  in.no_hard = flags & kNoHard;
  in.wave_kernel = flags & kWave;
  in.device_block = flags & kBlock;
  std::snprintf(context, sizeof(context), "N=%lld Dj=%d M=%d path=%d flags=%d cus=%d", (long long)N, Dj, M, path, flags, cus);
  return estep_plan(in);
}

// ---- (a) literal plans ----
static void check_table() {
  {  // one mixture tile: estep_small_kernel<80, 1>, 16-frame blocks, four workgroups per CU, two partial rows per workgroup.
     // The partial rows of estep_mfma_kernel over the same frames (16 workgroups x 8 waves per tile) are the larger reservation.
    const EstepPlan p = plan(1000, 80, 8);
    CHECK_EQ(p.route, kRouteMfma);
    CHECK_EQ(p.DJ, 80);
    CHECK_EQ(p.body, kBodySmall1);
    CHECK_EQ(p.mtp, 1);
    CHECK_EQ(p.wpt, 8);
    CHECK(p.share);
    CHECK_EQ(p.plen, 1289);
    CHECK_EQ(p.body_grid[0], 63);
    CHECK_EQ(p.body_rows[0], 126);
    CHECK_EQ(p.n_part, 128 * 1289);
    CHECK_EQ(p.reduce_grid, 21);
    CHECK_EQ(p.prep_grid, 80);
    CHECK_EQ(p.n_raw, 8 * 161);
    CHECK_EQ(p.n_Wpack, 8 * 40 * 64);
    CHECK_EQ(p.n_cinit, 128);
    CHECK_EQ(p.n_refiv, 640);
    CHECK_EQ(p.n_refc, 16);
    CHECK_EQ(p.chunks.count, 1);
    CHECK(!p.hard && !p.copy_down);
    CHECK_EQ(p.n_Xsoft + p.n_G + p.n_hkeys, 0);
  }
  {  // two mixture tiles: estep_small_kernel<80, 2>, 32-frame blocks, two workgroups per CU
    const EstepPlan p = plan(1000, 80, 17);
    CHECK_EQ(p.body, kBodySmall2);
    CHECK_EQ(p.mtp, 2);
    CHECK_EQ(p.wpt, 4);
    CHECK_EQ(p.plen, 2738);
    CHECK_EQ(p.body_grid[0], 32);
    CHECK_EQ(p.body_rows[0], 64);
    CHECK_EQ(p.n_part, 64 * 2738);
  }
  {
    const EstepPlan p = plan(1000, 80, 32);
    CHECK_EQ(p.body, kBodySmall2);
    CHECK_EQ(p.mtp, 2);
  }
  {  // 33 mixtures: the one-kernel body, three tiles rounded up to four, two waves per tile
    const EstepPlan p = plan(1000, 80, 33);
    CHECK_EQ(p.body, kBodyOne);
    CHECK(p.share);
    CHECK_EQ(p.mtp, 4);
    CHECK_EQ(p.wpt, 2);
    CHECK_EQ(p.body_grid[0], 16);
    CHECK_EQ(p.body_rows[0], 32);
    CHECK_EQ(p.n_part, 32 * (33 * 161 + 1));
    // rows of 82 doubles: two x buffers of 41 KB-instructions (5248 doubles), 64 x 144 of gamma, the exp table, 128 thresholds;
    // 9 x 64 ints of frame order
    CHECK_EQ(p.body_lds, (2 * 5248 + 64 * 144 + 64 + 128) * 8 + 9 * 64 * 4);
  }
  {
    const EstepPlan p = plan(1000, 80, 64);
    CHECK_EQ(p.mtp, 4);
    CHECK(p.share);
  }
  {  // 65 mixtures: eight tiles, every wave its own
    const EstepPlan p = plan(1000, 80, 65);
    CHECK_EQ(p.body, kBodyOne);
    CHECK(!p.share);
    CHECK_EQ(p.mtp, 8);
    CHECK_EQ(p.wpt, 1);
    CHECK_EQ(p.body_grid[0], 16);
    CHECK_EQ(p.body_rows[0], 16);
  }
  // ---- the hard-assignment chain: wanted from 65536 frames, below 2^31, unless pinned soft; one tile only when pinned hard ----
  CHECK(!plan(65535, 80, 32).hard);
  {
    const EstepPlan p = plan(65536, 80, 32);
    CHECK(p.hard && p.sample);
    CHECK_EQ(p.body, kBodySmall2);
    CHECK_EQ(p.soft_body, kBodySmall2);
    CHECK_EQ(p.nchunks, 64);
    CHECK_EQ(p.nsample, 16);
    CHECK_EQ(p.cstride, 4);
    CHECK_EQ(p.sample_grid, 64);
    CHECK_EQ(p.key_grid, 64);
    CHECK_EQ(p.npmax, 288);
    CHECK_EQ(p.MT, 2);
    CHECK_EQ(p.MK, 33);
    CHECK_EQ(p.key_lds, 2 * (5 * 2048 + 192) + 33 * 4);
    CHECK_EQ(p.gathered_grid, 512);
    CHECK_EQ(p.gathered_rows, 1024);
    CHECK_EQ(p.allsoft_grid, 512);
    CHECK_EQ(p.allsoft_rows, 1024);
    CHECK_EQ(p.n_part, 1024 * 5153);
  }
  CHECK(!plan(65536, 80, 16).hard);
  {
    const EstepPlan p = plan(65536, 80, 16, VCMI_ESTEP_HARD);
    CHECK(p.hard && !p.sample);
    CHECK_EQ(p.soft_body, kBodySmall1);
    CHECK_EQ(p.gathered_grid, 1024);
    CHECK_EQ(p.gathered_rows, 2048);
    CHECK_EQ(p.allsoft_grid, 0);
    CHECK_EQ(p.allsoft_rows, 0);
    CHECK_EQ(p.n_part, 2048 * (16 * 161 + 1));
  }
  CHECK(!plan(65536, 80, 16, VCMI_ESTEP_SOFT).hard);
  CHECK(!plan(65536, 80, 32, VCMI_ESTEP_SOFT).hard);
  CHECK(!plan(65536, 80, 16, VCMI_ESTEP_AUTO, kNoHard).hard);
  CHECK(!plan(65536, 80, 32, VCMI_ESTEP_HARD, kNoHard).hard);
  CHECK(plan(65536, 80, 16, VCMI_ESTEP_AUTO, kNoSmall).hard);       // (without the one-tile kernel there is something to decide)
  CHECK(!plan((int64_t)1 << 31, 80, 128).hard);
  CHECK(!plan((int64_t)1 << 31, 48, 40, VCMI_ESTEP_HARD).hard);
  CHECK(plan(((int64_t)1 << 31) - 1, 80, 128).hard);
  CHECK(!plan(100000, 82, 128, VCMI_ESTEP_HARD).hard);              // (the two-kernel form has no hard chain)
  {  // the benchmark's shape
    const EstepPlan p = plan(1250000, 80, 128);
    CHECK_EQ(p.route, kRouteMfma);
    CHECK(p.hard && p.sample);
    CHECK_EQ(p.nchunks, 1221);
    CHECK_EQ(p.nsample, 16);
    CHECK_EQ(p.cstride, 76);
    CHECK_EQ(p.sample_grid, 64);
    CHECK_EQ(p.key_grid, 256);
    CHECK_EQ(p.npmax, 5011);
    CHECK_EQ(p.prow, 162);
    CHECK_EQ(p.MT, 8);
    CHECK_EQ(p.MK, 129);
    CHECK_EQ(p.plen, 20609);
    CHECK_EQ(p.soft_body, kBodyOne);
    CHECK_EQ(p.body, kBodyOne);
    CHECK(!p.share);
    CHECK_EQ(p.gathered_grid, 256);
    CHECK_EQ(p.gathered_rows, 256);
    CHECK_EQ(p.allsoft_grid, 256);
    CHECK_EQ(p.allsoft_rows, 256);
    CHECK_EQ(p.body_grid[0], 256);
    CHECK_EQ(p.body_rows[0], 256);
    CHECK_EQ(p.hprep_grid, 42);
    CHECK_EQ(p.scan_grid, 129);
    CHECK_EQ(p.scatter_grid, 1221);
    CHECK_EQ(p.hstats_grid, 5011);
    CHECK_EQ(p.hreduce_grid, 128);
    CHECK_EQ(p.gather_grid, 1024);
    CHECK_EQ(p.key_lds, 8 * (5 * 2048 + 192) + 129 * 4);
    CHECK_EQ(p.scatter_lds, 17 * 129 * 4);
    CHECK_EQ(p.n_part, 256 * 20609);
    CHECK_EQ(p.n_Xsoft, 100000000);
    CHECK_EQ(p.n_W16, 8 * (5 * 2048 + 192));
    CHECK_EQ(p.n_probe, 64 * 129);
    CHECK_EQ(p.n_ctl, 4);
    CHECK_EQ(p.n_hkeys, 2 * 1250000 + 1222 * 129);
    CHECK_EQ(p.n_hpart, 5011 * 162);
    CHECK_EQ(p.n_hllm, 128);
  }
  // ---- the ladder of instantiated dimensions ----
  CHECK_EQ(plan(1000, 2, 8).DJ, 32);
  CHECK_EQ(plan(1000, 32, 8).DJ, 32);
  CHECK_EQ(plan(1000, 34, 8).DJ, 48);
  CHECK_EQ(plan(1000, 48, 8).DJ, 48);
  CHECK_EQ(plan(1000, 50, 8).DJ, 64);
  CHECK_EQ(plan(1000, 64, 8).DJ, 64);
  CHECK_EQ(plan(1000, 66, 8).DJ, 80);
  CHECK_EQ(plan(1000, 80, 8).DJ, 80);
  CHECK_EQ(plan(1000, 112, 8).DJ, 112);
  CHECK_EQ(plan(1000, 114, 8).DJ, 160);
  {  // above 80: the two-kernel form, 32-frame blocks, no small kernels
    const EstepPlan p = plan(1000, 82, 8);
    CHECK_EQ(p.DJ, 112);
    CHECK_EQ(p.body, kBodySplit);
    CHECK(p.share);
    CHECK_EQ(p.wpt, 8);
    CHECK_EQ(p.chunks.count, 1);
    CHECK_EQ(p.chunks.len, 1000);
    CHECK_EQ(p.body_grid[0], 32);
    CHECK_EQ(p.body_rows[0], 256);
    CHECK_EQ(p.body_grid[1], 32);
    CHECK_EQ(p.n_G, 1000 * 128);
    CHECK_EQ(p.n_part, 256 * (8 * 165 + 1));
    CHECK_EQ(p.prep_grid, 8 * 56 * 64 / 256);
  }
  {  // ... in chunks of 2^20 frames
    const EstepPlan p = plan(((int64_t)1 << 20) + 1, 160, 128);
    CHECK_EQ(p.DJ, 160);
    CHECK_EQ(p.body, kBodySplit);
    CHECK(!p.share);
    CHECK_EQ(p.chunks.len, 1 << 20);
    CHECK_EQ(p.chunks.count, 2);
    CHECK_EQ(p.chunks.last, 1);
    CHECK_EQ(p.body_grid[0], 256);
    CHECK_EQ(p.body_rows[0], 256);
    CHECK_EQ(p.body_grid[1], 1);
    CHECK_EQ(p.body_rows[1], 1);
    CHECK_EQ(p.n_G, (int64_t)128 << 20);
    CHECK_EQ(p.n_part, 256 * (128 * 321 + 1));
  }
  {  // odd: padded to the next even dimension, in chunks
    const EstepPlan p = plan(((int64_t)1 << 20) + 3, 81, 20);
    CHECK_EQ(p.route, kRoutePadOdd);
    CHECK_EQ(p.djp, 82);
    CHECK_EQ(p.plen_p, 20 * 165 + 1);
    CHECK_EQ(p.chunks.count, 2);
    CHECK_EQ(p.chunks.last, 3);
    CHECK_EQ(p.pad_grid[0], 65536);
    CHECK_EQ(p.pad_grid[1], 1);
    CHECK_EQ(p.unpad_grid, 7);
    CHECK_EQ(p.n_Xpad, (int64_t)82 << 20);
    CHECK_EQ(p.n_statsp, 3301);
    CHECK_EQ(plan(p.chunks.len, p.djp, 20).DJ, 112);
    CHECK_EQ(plan(100, 159, 20).route, kRoutePadOdd);
    CHECK_EQ(plan(100, 159, 20).djp, 160);
    CHECK_EQ(plan(100, 1, 1).route, kRoutePadOdd);
  }
  CHECK_EQ(plan(1000, 161, 8).route, kRouteGeneric);
  {
    const EstepPlan p = plan(65537, 162, 3);
    CHECK_EQ(p.route, kRouteGeneric);
    CHECK_EQ(p.chunks.len, 65536);
    CHECK_EQ(p.chunks.count, 2);
    CHECK_EQ(p.chunks.last, 1);
    CHECK_EQ(p.gamma_grid[0], 1024);
    CHECK_EQ(p.gamma_grid[1], 1);
    CHECK_EQ(p.nseg[0], 128);
    CHECK_EQ(p.nseg[1], 1);
    CHECK_EQ(p.stats_grid_y, 2);
    CHECK_EQ(p.gamma_lds, 162 * 512);
    CHECK_EQ(p.plen, 976);
    CHECK_EQ(p.n_part, 128 * 976);
    CHECK_EQ(p.n_G, 65536 * 3);
    CHECK_EQ(p.n_LSE, 65536);
    CHECK_EQ(p.n_mu, 486);
    CHECK_EQ(p.n_cst, 3);
  }
  {  // more than 128 mixtures: groups of 128
    const EstepPlan p = plan(1000, 80, 129);
    CHECK_EQ(p.route, kRouteGroups);
    CHECK_EQ(p.ng, 2);
    CHECK_EQ(p.Mg_last, 1);
    CHECK_EQ(p.DJ, 80);
    CHECK_EQ(p.chunks.count, 1);
    CHECK_EQ(p.group_grid[0], 16);
    CHECK_EQ(p.group_reduce_grid[0], 81);
    CHECK_EQ(p.group_reduce_grid[1], 1);
    CHECK_EQ(p.prep_grid, 80);
    CHECK_EQ(p.n_Wpack, 2 * 8 * 40 * 64);
    CHECK_EQ(p.n_cinit, 256);
    CHECK_EQ(p.n_raw, 129 * 161);
    CHECK_EQ(p.n_G, 2 * 1000 * 128);
    CHECK_EQ(p.n_LSE, 2 * 1000 + 1024);
    CHECK_EQ(p.n_part, 256 * 20609);
    CHECK(!p.hard && !p.copy_down);
    const EstepPlan q = plan(((int64_t)1 << 18) + 5, 160, 257);
    CHECK_EQ(q.ng, 3);
    CHECK_EQ(q.Mg_last, 1);
    CHECK_EQ(q.chunks.count, 2);
    CHECK_EQ(q.chunks.last, 5);
    CHECK_EQ(q.group_grid[0], 256);
    CHECK_EQ(q.group_grid[1], 1);
  }
  // ---- the test hooks ----
  CHECK_EQ(plan(1000, 80, 64, VCMI_ESTEP_AUTO, kWave).body, kBodyOne);
  {
    const EstepPlan p = plan(1000, 80, 65, VCMI_ESTEP_AUTO, kWave);
    CHECK_EQ(p.body, kBodyWave);
    CHECK_EQ(p.body_grid[0], 32);
    CHECK_EQ(p.body_rows[0], 32);
    CHECK_EQ(p.n_part, 32 * (65 * 161 + 1));
    // behind a hard chain the FP64 launches stay the three-barrier kernel; the wave kernel is what a demoted chain runs
    const EstepPlan q = plan(70000, 80, 65, VCMI_ESTEP_AUTO, kWave);
    CHECK(q.hard);
    CHECK_EQ(q.body, kBodyWave);
    CHECK_EQ(q.soft_body, kBodyOne);
    CHECK_EQ(plan(1000, 112, 65, VCMI_ESTEP_AUTO, kWave).body, kBodySplit);
  }
  {
    const EstepPlan p = plan(1000, 80, 8, VCMI_ESTEP_AUTO, kGeneric);
    CHECK_EQ(p.route, kRouteGeneric);
    CHECK_EQ(p.gamma_grid[0], 16);
    CHECK_EQ(p.nseg[0], 2);
    CHECK_EQ(p.stats_grid_y, 3);
    CHECK_EQ(p.n_part, 2 * 1289);
    CHECK_EQ(plan(1000, 81, 8, VCMI_ESTEP_AUTO, kGeneric).route, kRouteGeneric);
    CHECK_EQ(plan(1000, 80, 200, VCMI_ESTEP_AUTO, kGeneric).route, kRouteGeneric);
  }
  for (int M : {8, 17, 32}) {
    const EstepPlan p = plan(1000, 80, M, VCMI_ESTEP_AUTO, kNoSmall);
    CHECK_EQ(p.body, kBodyOne);
    CHECK(p.share);
    CHECK_EQ(p.body_grid[0], 16);
    CHECK_EQ(p.body_rows[0], 16 * (M <= 16 ? 8 : 4));
  }
  // ---- a device parameter block stays on the device exactly where estep_mfma_launch serves the shape ----
  CHECK(!plan(1000, 80, 128, VCMI_ESTEP_AUTO, kBlock).copy_down);
  CHECK(!plan(1000, 160, 1, VCMI_ESTEP_AUTO, kBlock).copy_down);
  CHECK(plan(1000, 80, 129, VCMI_ESTEP_AUTO, kBlock).copy_down);
  CHECK(plan(1000, 79, 8, VCMI_ESTEP_AUTO, kBlock).copy_down);
  CHECK(plan(1000, 162, 8, VCMI_ESTEP_AUTO, kBlock).copy_down);
  CHECK(plan(1000, 80, 8, VCMI_ESTEP_AUTO, kBlock | kGeneric).copy_down);
  CHECK(!plan(1000, 80, 129).copy_down);
}

// ---- (b) properties ----
static bool fits_int(long long v) { return v >= 0 && v < (1ll << 31); }

static void check_properties(int64_t N, int Dj, int M, int path, int flags, int cus) {
  const EstepPlan p = plan(N, Dj, M, path, flags, cus);
  CHECK_EQ(p.plen, (int64_t)M * (1 + 2 * Dj) + 1);
  CHECK(p.reduce_grid >= 1 && (int64_t)p.reduce_grid * 64 >= p.plen);
  CHECK(p.chunks.count >= 1 && p.chunks.len >= 1 && p.chunks.last >= 1 && p.chunks.last <= p.chunks.len);
  CHECK_EQ((p.chunks.count - 1) * p.chunks.len + p.chunks.last, N);
  CHECK_EQ(p.copy_down, (flags & kBlock) && p.route != kRouteMfma);
  for (size_t n : {p.n_part, p.n_G, p.n_LSE, p.n_mu, p.n_cst, p.n_Xpad, p.n_statsp, p.n_raw, p.n_Wpack, p.n_cinit, p.n_refiv, p.n_refc, p.n_Xsoft,
                   p.n_W16, p.n_probe, p.n_ctl, p.n_hkeys, p.n_hpart, p.n_hllm})
    CHECK(n < ((size_t)1 << 40));       // (nothing wrapped around)
  const int64_t nfr[2] = {p.chunks.len, p.chunks.last};
  switch (p.route) {
    case kRouteGeneric:
      CHECK((flags & kGeneric) || Dj > 160);
      for (int i = 0; i < 2; ++i) {
        CHECK(p.gamma_grid[i] >= 1 && (int64_t)p.gamma_grid[i] * 64 >= nfr[i]);
        CHECK(p.nseg[i] >= 1 && (int64_t)p.nseg[i] * kSeg >= nfr[i]);
        CHECK(p.n_part >= (size_t)p.nseg[i] * p.plen);
      }
      CHECK(p.stats_grid_y >= 1 && p.stats_grid_y * 256 >= M * Dj);
      CHECK(p.n_G >= (size_t)p.chunks.len * M && p.n_LSE >= (size_t)p.chunks.len);
      CHECK(p.n_mu == (size_t)M * Dj && p.n_cst == (size_t)M);
      CHECK_EQ(p.gamma_lds, (size_t)Dj * 512);
      break;
    case kRoutePadOdd: {
      CHECK(Dj % 2 == 1 && Dj < 160 && !(flags & kGeneric));
      CHECK_EQ(p.djp, Dj + 1);
      CHECK_EQ(p.plen_p, (int64_t)M * (1 + 2 * p.djp) + 1);
      for (int i = 0; i < 2; ++i) CHECK(p.pad_grid[i] >= 1 && p.pad_grid[i] <= 65536);
      CHECK(p.unpad_grid >= 1 && (int64_t)p.unpad_grid * 256 >= (int64_t)M * Dj);
      CHECK(p.n_Xpad >= (size_t)p.chunks.len * p.djp && p.n_statsp >= (size_t)p.plen_p);
      // every chunk is planned again, and that plan is never another padding
      for (int i = 0; i < 2; ++i) {
        const EstepPlan q = plan(nfr[i], p.djp, M, path, flags & ~kBlock, cus);
        CHECK(q.route == kRouteMfma || q.route == kRouteGroups);
        CHECK_EQ(q.plen, p.plen_p);
      }
      break;
    }
    case kRouteGroups:
      CHECK(M > 128 && Dj % 2 == 0 && Dj <= 160);
      CHECK(p.DJ >= Dj);
      CHECK_EQ((p.ng - 1) * 128 + p.Mg_last, M);
      CHECK(p.Mg_last >= 1 && p.Mg_last <= 128 && p.prep_grid >= 1);
      for (int i = 0; i < 2; ++i) {
        CHECK(p.group_grid[i] >= 1 && p.group_grid[i] <= cus);
        CHECK(p.n_part >= (size_t)p.group_grid[i] * ((size_t)128 * (1 + 2 * Dj) + 1));      // rows of a whole group
        CHECK(p.group_reduce_grid[i] >= 1);
      }
      CHECK((int64_t)p.group_reduce_grid[0] * 256 >= (int64_t)128 * (1 + 2 * Dj));
      CHECK((int64_t)p.group_reduce_grid[1] * 256 >= (int64_t)p.Mg_last * (1 + 2 * Dj));
      CHECK(p.n_G >= (size_t)p.ng * p.chunks.len * 128 && p.n_LSE >= (size_t)p.ng * p.chunks.len + kCombineGrid);
      CHECK(p.n_Wpack >= (size_t)p.ng * 256 * p.DJ && p.n_cinit >= (size_t)128 * p.ng);
      CHECK(p.n_raw == (size_t)M * (1 + 2 * Dj) && p.n_refiv >= (size_t)M * Dj && p.n_refc >= (size_t)2 * M);
      CHECK(!p.hard);
      break;
    case kRouteMfma: {
      CHECK(M <= 128 && Dj % 2 == 0 && Dj <= 160 && !(flags & kGeneric));
      CHECK(p.DJ >= Dj && p.DJ == estep_mfma_dj(Dj));
      CHECK(16 * p.mtp >= M && (p.mtp == 1 || 8 * p.mtp < M) && p.mtp * p.wpt == 8 && p.share == (p.mtp < 8));
      CHECK(p.prep_grid >= 1 && (size_t)p.prep_grid * 256 >= p.n_Wpack && p.prep_grid * 256 >= 16 * 128 && (size_t)p.prep_grid * 256 >= p.n_refiv);
      CHECK(p.n_Wpack == (size_t)256 * p.DJ && p.n_cinit >= 128 && p.n_raw == (size_t)M * (1 + 2 * Dj));
      CHECK(p.n_refiv >= (size_t)M * Dj && p.n_refc >= (size_t)2 * M);
      CHECK(p.body_lds > 0 && p.body_lds <= 160 * 1024);
      for (int i = 0; i < 2; ++i) {
        CHECK(p.body_grid[i] >= 1 && p.body_rows[i] >= p.body_grid[i]);
        CHECK(p.n_part >= (size_t)p.body_rows[i] * p.plen);
      }
      CHECK_EQ(p.body == kBodySplit, p.DJ > 80);
      if (p.body == kBodySplit) {
        CHECK(p.n_G >= (size_t)p.chunks.len * 128);
        CHECK(!p.hard);
      } else {
        CHECK_EQ(p.chunks.count, 1);
        CHECK_EQ(p.body == kBodyWave, (flags & kWave) && M > 64);
        const bool small = M <= 32 && !(flags & kNoSmall);
        CHECK_EQ(p.soft_body, !small ? kBodyOne : M <= 16 ? kBodySmall1 : kBodySmall2);
        if (p.body != kBodyWave) CHECK_EQ(p.body, p.soft_body);
      }
      if (p.hard) {
        CHECK(N >= 65536 && N < (1ll << 31) && path != VCMI_ESTEP_SOFT && !(flags & kNoHard));
        CHECK_EQ(p.sample, path == VCMI_ESTEP_AUTO);
        CHECK(p.nsample >= 1 && p.nsample <= 16 && p.cstride >= 1 && (p.nsample - 1) * p.cstride < p.nchunks);
        CHECK(p.nchunks * kHardChunk >= N && (p.nchunks - 1) * kHardChunk < N);
        CHECK_EQ(p.MK, M + 1);
        CHECK_EQ(p.MT, (M + 15) / 16);
        CHECK_EQ(p.prow, 2 * Dj + 2);
        CHECK(p.n_hkeys >= (size_t)2 * N + (size_t)(p.nchunks + 1) * p.MK);
        CHECK(p.n_hpart >= (size_t)p.npmax * p.prow && p.n_hllm >= (size_t)M && p.n_ctl >= (size_t)kCtlLen);
        CHECK(p.n_probe >= (size_t)p.sample_grid * p.MK && p.n_Xsoft >= (size_t)N * Dj);
        CHECK(p.n_W16 + (size_t)p.MK * 4 == p.key_lds && p.key_lds <= 160 * 1024);
        CHECK_EQ(p.scatter_lds, (size_t)17 * p.MK * 4);
        // pieces of 256 hard frames per owner, for some assignments of the N frames to the M owners: all to one, spread evenly,
        // one frame each and the rest to the last
        const int64_t even = N / M, rest = N - even * M;
        int64_t pieces_even = 0;
        for (int m = 0; m < M; ++m) pieces_even += (even + (m < rest ? 1 : 0) + kHardPiece - 1) / kHardPiece;
        const int64_t pieces_one = (N + kHardPiece - 1) / kHardPiece, pieces_tail = (M - 1) + (N - (M - 1) + kHardPiece - 1) / kHardPiece;
        CHECK(p.npmax >= pieces_even && p.npmax >= pieces_one && p.npmax >= pieces_tail);
        CHECK(p.npmax >= N / kHardPiece + M);       // (the bound: sum_m ceil(n_m / 256) <= sum_m (n_m / 256 + 1))
        for (int g : {p.hprep_grid, p.sample_grid, p.key_grid, p.scan_grid, p.scatter_grid, p.hstats_grid, p.hreduce_grid, p.gather_grid,
                      p.gathered_grid})
          CHECK(g >= 1);
        CHECK(p.key_grid <= cus && p.sample_grid == p.nsample * kHardSamplePasses && p.scatter_grid == p.nchunks && p.hstats_grid == p.npmax);
        CHECK(p.hprep_grid * 256 >= p.MT * ((p.DJ + 15) / 16) * 64 + 256 * 4 * p.MT);
        CHECK(p.n_part >= (size_t)p.gathered_rows * p.plen && p.gathered_rows >= p.gathered_grid);
        if (p.sample) CHECK(p.allsoft_grid >= 1 && p.allsoft_rows >= p.allsoft_grid && p.n_part >= (size_t)p.allsoft_rows * p.plen);
        CHECK(fits_int(p.npmax) && fits_int(p.nchunks) && fits_int((long long)p.key_lds) && fits_int((long long)p.nsample * kHardSamplePasses));
      } else {
        CHECK_EQ(p.n_Xsoft + p.n_W16 + p.n_probe + p.n_ctl + p.n_hkeys + p.n_hpart + p.n_hllm, 0);
      }
      break;
    }
  }
  for (long long v : {(long long)p.reduce_grid, (long long)p.gamma_grid[0], (long long)p.gamma_grid[1], (long long)p.nseg[0], (long long)p.nseg[1],
                      (long long)p.stats_grid_y, (long long)p.djp, (long long)p.pad_grid[0], (long long)p.pad_grid[1], (long long)p.unpad_grid,
                      (long long)p.DJ, (long long)p.prep_grid, (long long)p.ng, (long long)p.Mg_last, (long long)p.group_grid[0],
                      (long long)p.group_grid[1], (long long)p.group_reduce_grid[0], (long long)p.group_reduce_grid[1], (long long)p.mtp,
                      (long long)p.wpt, (long long)p.body_grid[0], (long long)p.body_grid[1], (long long)p.body_rows[0], (long long)p.body_rows[1],
                      (long long)p.gathered_grid, (long long)p.gathered_rows, (long long)p.allsoft_grid, (long long)p.allsoft_rows, (long long)p.MT,
                      (long long)p.MK, (long long)p.hprep_grid, (long long)p.sample_grid, (long long)p.key_grid, (long long)p.scan_grid,
                      (long long)p.scatter_grid, (long long)p.hstats_grid, (long long)p.hreduce_grid, (long long)p.gather_grid,
                      (long long)p.plen, (long long)p.plen_p})
    CHECK(fits_int(v));
}

// ---- the launch sequence a plan stands for, one line per kernel: name, grid in work-items (x, y), workgroup size -- the form
// of a kernel trace, so that what a device ran can be compared with the plan (`estep_plan_check --sequence N Dj M path flags
// cus`, flags as enum Flag; host parameters) ----
static void line(const char *name, long long grid, int wg, int grid_y = 1) { std::printf("%s grid=%lldx%d wg=%d\n", name, grid * wg, grid_y, wg); }
static void fmt(char *buf, size_t n, const char *pattern, int DJ, int a = 0, bool share = false) {
  std::snprintf(buf, n, pattern, DJ, a, share ? "true" : "false");
}
static void print_soft(const EstepPlan &p, EstepBody body, int grid) {
  char k[64];
  if (body == kBodyOne) fmt(k, sizeof(k), "estep_mfma_kernel<%d, %d, %s>", p.DJ, 0, p.share);
  else fmt(k, sizeof(k), "estep_small_kernel<%d, %d>", p.DJ, body == kBodySmall1 ? 1 : 2);
  line(k, grid, body == kBodyOne ? 512 : body == kBodySmall1 ? 128 : 256);
  line("estep_reduce_kernel", p.reduce_grid, 256);
}
static void print_sequence(const EstepPlanInput &in) {
  const EstepPlan p = estep_plan(in);
  char k[64];
  switch (p.route) {
    case kRouteGeneric:
      for (int64_t i = 0; i < p.chunks.count; ++i) {
        const bool last = i == p.chunks.count - 1;
        line("estep_gamma_kernel", p.gamma_grid[last], 64);
        line("estep_stats_kernel", p.nseg[last], 256, p.stats_grid_y);
        line("estep_reduce_kernel", p.reduce_grid, 256);
      }
      break;
    case kRoutePadOdd:
      for (int64_t i = 0; i < p.chunks.count; ++i) {
        const bool last = i == p.chunks.count - 1;
        EstepPlanInput inner = in;
        inner.N = last ? p.chunks.last : p.chunks.len;
        inner.Dj = p.djp;
        line("estep_pad_x_kernel", p.pad_grid[last], 256);
        print_sequence(inner);
        line("estep_unpad_stats_kernel", p.unpad_grid, 256);
      }
      break;
    case kRouteGroups:
      line("estep_param_copy_kernel", (long long)(p.n_raw + 255) / 256, 256);
      fmt(k, sizeof(k), "estep_prep_kernel<%d>", p.DJ);
      for (int g = 0; g < p.ng; ++g) line(k, p.prep_grid, 256);
      for (int64_t i = 0; i < p.chunks.count; ++i) {
        const bool last = i == p.chunks.count - 1;
        fmt(k, sizeof(k), "estep_mfma_kernel<%d, %d, %s>", p.DJ, 3, false);
        for (int g = 0; g < p.ng; ++g) line(k, p.group_grid[last], 512);
        line("estep_group_combine_kernel", kCombineGrid, 256);
        line("estep_sum_kernel", 1, 256);
        fmt(k, sizeof(k), "estep_mfma_kernel<%d, %d, %s>", p.DJ, 2, false);
        for (int g = 0; g < p.ng; ++g) {
          line(k, p.group_grid[last], 512);
          line("estep_group_reduce_kernel", p.group_reduce_grid[g == p.ng - 1], 256);
        }
      }
      break;
    case kRouteMfma:
      line("estep_param_copy_kernel", (long long)(p.n_raw + 255) / 256, 256);
      fmt(k, sizeof(k), "estep_prep_kernel<%d>", p.DJ);
      line(k, p.prep_grid, 256);
      if (p.body == kBodySplit) {
        for (int64_t i = 0; i < p.chunks.count; ++i) {
          const bool last = i == p.chunks.count - 1;
          for (int phase : {1, 2}) {
            fmt(k, sizeof(k), "estep_mfma_kernel<%d, %d, %s>", p.DJ, phase, p.share);
            line(k, p.body_grid[last], 512);
          }
          line("estep_reduce_kernel", p.reduce_grid, 256);
        }
      } else if (p.hard) {
        fmt(k, sizeof(k), "estep_hard_prep_kernel<%d>", p.DJ);
        line(k, p.hprep_grid, 256);
        fmt(k, sizeof(k), "estep_hard_key_kernel<%d>", p.DJ);
        if (p.sample) line(k, p.sample_grid, kHardKeyThreads);
        line("estep_path_decide_kernel", 1, 1024);
        line(k, p.key_grid, kHardKeyThreads);
        line("gmmmap_group_scan_kernel", p.scan_grid, 256);
        line("gmmmap_group_scatter_kernel", p.scatter_grid, 256);
        fmt(k, sizeof(k), "estep_hard_stats_kernel<%d>", p.DJ);
        line(k, p.hstats_grid, 256);
        line("estep_hard_reduce_kernel", p.hreduce_grid, 256);
        line("estep_hard_ll_kernel", 1, 64);
        line("estep_hard_gather_kernel", p.gather_grid, 256);
        print_soft(p, p.soft_body, p.gathered_grid);
        if (p.sample) print_soft(p, p.soft_body, p.allsoft_grid);
      } else if (p.body == kBodyWave) {
        fmt(k, sizeof(k), "estep_wave_kernel<%d>", p.DJ);
        line(k, p.body_grid[0], 512);
        line("estep_reduce_kernel", p.reduce_grid, 256);
      } else {
        print_soft(p, p.body, p.body_grid[0]);
      }
      break;
  }
}

int main(int argc, char **argv) {
  if (argc == 8 && std::string(argv[1]) == "--sequence") {
    EstepPlanInput in;
    in.N = std::atoll(argv[2]);
    in.Dj = std::atoi(argv[3]);
    in.M = std::atoi(argv[4]);
    in.path = std::atoi(argv[5]);
    const int flags = std::atoi(argv[6]);
    in.cus = std::atoi(argv[7]);
    in.generic = flags & kGeneric;
    in.no_small = flags & kNoSmall;
    in.no_hard = flags & kNoHard;
    in.wave_kernel = flags & kWave;
    print_sequence(in);
    return 0;
  }
  check_table();
  long long plans = 0;
  for (int Dj = 2; Dj <= 164; ++Dj)
    for (int M : {1, 16, 17, 32, 33, 64, 65, 128, 129, 257})
      for (int64_t N : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)65535, (int64_t)65536, ((int64_t)1 << 20) + 1})
        for (int cus : {1, 256, 304}) {
          for (int path : {VCMI_ESTEP_AUTO, VCMI_ESTEP_HARD, VCMI_ESTEP_SOFT}) {
            check_properties(N, Dj, M, path, kNone, cus);
            ++plans;
          }
          for (int flags : {(int)kGeneric, (int)kNoSmall, (int)kNoHard, (int)kWave, (int)kBlock, kNoSmall | kWave | kBlock}) {
            check_properties(N, Dj, M, VCMI_ESTEP_AUTO, flags, cus);
            ++plans;
          }
          check_properties(N, Dj, M, VCMI_ESTEP_HARD, kNoSmall | kWave, cus);
          ++plans;
        }
  // frame counts around 2^31: the hard chain's int frame indices end there
  for (int64_t N : {((int64_t)1 << 31) - 1, (int64_t)1 << 31, ((int64_t)1 << 31) + 1})
    for (int Dj : {32, 80, 81, 160, 162})
      for (int M : {16, 128, 129}) {
        check_properties(N, Dj, M, VCMI_ESTEP_HARD, kNone, 256);
        ++plans;
      }
  if (failures) {
    std::printf("estep_plan_check: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("estep_plan_check: ok (%lld plans)\n", plans);
  return 0;
}
