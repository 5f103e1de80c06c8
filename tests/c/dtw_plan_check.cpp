// dtw_plan_check.cpp -- exact facts about the job list of the fused DTW path (csrc/dtw_plan.cpp): pair order and offsets, how
// the jobs tile the descriptors, how the strips tile the rows and the segments the columns, and the flag wiring -- above all
// that a job waits only on flags signalled by a STRICTLY EARLIER job, the property that keeps the persistent kernel
// (dtw_fused_persistent_kernel) free of deadlock.  Six batches x slots {2, 8, 24, 48, 64, 512} x the four settings of the test hooks
// (small slot counts are what cuts small batches into segments),
// plus three plans with hand-written descriptors.  Stand-alone (no device, no HIP); tests/test_dtw_plan_host.py builds it with
// ASan + UBSan and runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../../voiceconversion.jl_amd/csrc/dtw_plan.hpp"

using namespace vcmi;

static int failures = 0;
static const char *context = "";
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      if (++failures <= 50) std::printf("FAILED %s:%d [%s]: %s\n", __FILE__, __LINE__, context, #cond); \
    }                                                                                \
  } while (0)

static uint64_t rng_state = 1;
static int draw(int lo, int hi) {      // uniform in [lo, hi], a fixed sequence
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (int)((rng_state >> 33) % (uint64_t)(hi - lo + 1));
}

static double some_newtgt;             // never dereferenced: "this pair wants newtgt"

// tmpl_off carries the caller's index, so that the sorted list can be checked against the input
static std::vector<DtwPair> make_pairs(const std::vector<std::pair<int, int>> &shapes, bool align) {
  std::vector<DtwPair> pairs;
  for (size_t i = 0; i < shapes.size(); ++i) {
    DtwPair p{};
    p.tmpl_off = (int64_t)i;
    p.S = shapes[i].first;
    p.T = shapes[i].second;
    p.newtgt = (align && i % 3 == 1) ? &some_newtgt : nullptr;
    pairs.push_back(p);
  }
  return pairs;
}

std::vector<std::vector<std::pair<int, int>>> dtw_plan_check_batches() {
  std::vector<std::vector<std::pair<int, int>>> b(6);
  // every strip count up to four, one row over and under each limit, T = 0 / 1 / not a multiple of 16
  b[0] = {{1, 7}, {9, 1}, {3, 0}, {512, 160}, {513, 97}, {549, 130}, {1025, 70}, {1537, 40}, {127, 500}, {128, 17},
          {129, 16}, {2, 300}, {640, 1}, {641, 16}, {1024, 17}};
  rng_state = 77;
  for (int i = 0; i < 1000; ++i) b[1].push_back({draw(450, 550), draw(450, 550)});       // the benchmark batch
  // the distribution of tests/test_gpu_dtw.py::test_column_segments_and_persistent_workgroups (602 pairs)
  for (int i = 0; i < 560; ++i) b[2].push_back({draw(100, 499), draw(130, 329)});
  for (int i = 0; i < 30; ++i) b[2].push_back({draw(513, 639), draw(130, 299)});         // packed bottom + upper
  for (int i = 0; i < 10; ++i) b[2].push_back({draw(700, 999), draw(130, 259)});         // wide bottom + upper
  b[2].push_back({1100, 143});
  b[2].push_back({1537, 131});                                                           // three / four strips
  // ... and of test_fused_kernel_more_workgroups_than_slots (740 pairs)
  for (int i = 0; i < 700; ++i) b[3].push_back({draw(20, 139), draw(20, 89)});
  for (int i = 0; i < 40; ++i) b[3].push_back({draw(513, 699), draw(20, 59)});
  // packed bottoms whose number is not a multiple of four (the T = 0 pair has no strip)
  for (int i = 0; i < 50; ++i) b[4].push_back({draw(513, 640), draw(100, 400)});
  b[4].push_back({600, 0});
  for (int i = 0; i < 40; ++i) b[5].push_back({draw(1, 2200), draw(0, 700)});
  return b;
}

struct StripKey {
  int pair, row0;
  bool operator<(const StripKey &o) const { return pair != o.pair ? pair < o.pair : row0 < o.row0; }
};

static void check_plan(const std::vector<DtwPair> &input, int row_len, int slots, bool segments_allowed, bool two_segments_max,
                       bool whole_first) {
  std::vector<DtwPair> pairs = input;
  const DtwFusedPlan plan = dtw_fused_plan(pairs, row_len, slots, segments_allowed, two_segments_max, whole_first);
  const std::vector<DtwStrip> &strips = plan.strips;
  const size_t n = pairs.size();

  // 1. pairs: a stable sort of the input by S*T, largest first; offsets are running sums; totals
  CHECK(n == input.size());
  {
    std::vector<char> seen(input.size(), 0);
    size_t ncodes = 0, nclast = 0, npath = 0, padn = 0;
    bool any_align = false;
    for (size_t k = 0; k < n; ++k) {
      const DtwPair &p = pairs[k];
      const size_t idx = (size_t)p.tmpl_off;
      CHECK(idx < input.size() && !seen[idx]);
      if (idx < input.size()) {
        seen[idx] = 1;
        CHECK(p.S == input[idx].S && p.T == input[idx].T && p.newtgt == input[idx].newtgt);
      }
      if (k > 0) {
        const int64_t a = (int64_t)pairs[k - 1].S * pairs[k - 1].T, b = (int64_t)p.S * p.T;
        CHECK(a >= b);
        if (a == b) CHECK(pairs[k - 1].tmpl_off < p.tmpl_off);
      }
      CHECK(p.fcodes_off == (int64_t)ncodes && p.clast_off == (int64_t)nclast && p.path32_off == (int64_t)npath);
      CHECK(p.spad_off == (int64_t)padn && p.tpad_off == (int64_t)(padn + (size_t)p.T * row_len));
      ncodes += (size_t)((p.T + 15) / 16) * (size_t)((p.S + 1) & ~1);
      nclast += (size_t)p.S;
      npath += (size_t)p.T;
      padn += (size_t)(p.T + p.S) * row_len;
      any_align = any_align || p.newtgt;
    }
    CHECK(plan.ncodes == ncodes && plan.nclast == nclast && plan.npath == npath && plan.padn == padn);
    CHECK(plan.any_align == any_align);
  }
  CHECK(plan.nseg == 1 || plan.nseg == 2 || plan.nseg == 3 || plan.nseg == 4 || plan.nseg == 5 || plan.nseg == 6 || plan.nseg == 8);
  if (!segments_allowed) CHECK(plan.nseg == 1);
  if (two_segments_max) CHECK(plan.nseg <= 2);
  CHECK(plan.nflags >= 0);

  // 2. jobs: one descriptor, or the four of a packed group; they tile `strips`; none is empty
  const size_t njobs = plan.job_first.size();
  CHECK(strips.empty() == plan.job_first.empty());
  std::vector<int> job_of(strips.size(), -1);
  for (size_t j = 0; j < njobs; ++j) {
    const int first = plan.job_first[j];
    const int end = j + 1 < njobs ? plan.job_first[j + 1] : (int)strips.size();
    CHECK(first == (j == 0 ? 0 : plan.job_first[j - 1] + (strips[(size_t)plan.job_first[j - 1]].packed ? 4 : 1)));
    CHECK(first >= 0 && first < end && end <= (int)strips.size());
    if (!(first >= 0 && first < end && end <= (int)strips.size())) return;
    CHECK(end - first == (strips[(size_t)first].packed ? 4 : 1));
    bool any = false;
    for (int d = first; d < end; ++d) {
      job_of[(size_t)d] = (int)j;
      CHECK((strips[(size_t)d].packed != 0) == (strips[(size_t)first].packed != 0));
      any = any || strips[(size_t)d].ncol > 0;
    }
    CHECK(any);
  }
  for (int j : job_of) CHECK(j >= 0);

  // the producer of every flag: its descriptor (one at most)
  std::vector<int> producer((size_t)plan.nflags, -1);
  for (size_t d = 0; d < strips.size(); ++d) {
    const DtwStrip &s = strips[d];
    CHECK(s.flag_out >= -1 && s.flag_out < plan.nflags);
    if (s.flag_out < 0 || s.flag_out >= plan.nflags) continue;
    CHECK(producer[(size_t)s.flag_out] < 0);
    producer[(size_t)s.flag_out] = (int)d;
    CHECK(s.ncol > 0);
  }
  if (!whole_first)
    for (int d : producer) CHECK(d >= 0);

  // 3. rows, 4. columns: the descriptors of every strip, in job order
  std::map<StripKey, std::vector<int>> of_strip;
  for (size_t d = 0; d < strips.size(); ++d) {
    const DtwStrip &s = strips[d];
    CHECK(s.pair >= 0 && (size_t)s.pair < n);
    if (!(s.pair >= 0 && (size_t)s.pair < n)) return;
    if (s.nrows == 0) {                    // padding of a packed group
      CHECK(s.packed != 0 && s.ncol == 0 && s.flag_in == -1 && s.flag_out == -1 && s.flag_prev == -1);
      continue;
    }
    CHECK(s.nrows > 0 && s.row0 >= 0 && s.ncol >= 0);
    CHECK(pairs[(size_t)s.pair].T > 0);
    if (s.ncol == 0) CHECK(s.packed != 0);   // only a packed group carries a strip whose segment is empty
    of_strip[StripKey{s.pair, s.row0}].push_back((int)d);
  }
  std::vector<std::vector<StripKey>> strips_of(n);
  for (const auto &kv : of_strip) strips_of[(size_t)kv.first.pair].push_back(kv.first);   // (increasing row0)
  std::vector<std::pair<int64_t, int64_t>> bnd_ranges;
  for (size_t k = 0; k < n; ++k) {
    const DtwPair &p = pairs[k];
    const std::vector<StripKey> &keys = strips_of[k];
    if (p.T == 0) {
      CHECK(keys.empty());
      continue;
    }
    CHECK((int)keys.size() == (p.S + kFusedRows - 1) / kFusedRows);
    int row = 0;
    for (size_t q = 0; q < keys.size(); ++q) {
      const std::vector<int> &ds = of_strip[keys[q]];
      const DtwStrip &s0 = strips[(size_t)ds[0]];
      const bool top = q + 1 == keys.size();
      CHECK(s0.row0 == row && s0.nrows <= kFusedRows);
      row += s0.nrows;
      if (top) CHECK(s0.bnd_out < 0);
      else CHECK(s0.nrows % 2 == 0 && s0.bnd_out >= 0);
      CHECK((s0.bnd_in >= 0) == (s0.row0 > 0));
      if (s0.packed) CHECK(s0.nrows <= 128 && s0.row0 == 0 && s0.flag_in < 0 && s0.bnd_in < 0);
      if (s0.bnd_out >= 0) {
        CHECK(s0.bnd_out + 2 * (int64_t)p.T <= (int64_t)plan.nbnd);
        bnd_ranges.push_back({s0.bnd_out, s0.bnd_out + 2 * (int64_t)p.T});
      }
      int col = 0, prev_flag_out = -1;
      bool first = true;
      for (int d : ds) {
        const DtwStrip &s = strips[(size_t)d];
        // every descriptor of the strip describes the same rows
        CHECK(s.nrows == s0.nrows && s.bnd_in == s0.bnd_in && s.bnd_out == s0.bnd_out && (s.packed != 0) == (s0.packed != 0));
        if (s.ncol == 0) continue;
        CHECK(s.col0 == col && s.col0 % 16 == 0);
        col = s.col0 + s.ncol;
        // 5. flag_prev: the previous non-empty segment of the strip
        CHECK(s.flag_prev == prev_flag_out && (s.flag_prev < 0) == first);
        CHECK((s.flag_out >= 0) == (s.bnd_out >= 0 || s.col0 + s.ncol < p.T));
        prev_flag_out = s.flag_out;
        first = false;
        // flag_in: the same segment of the strip below
        CHECK((s.flag_in >= 0) == (s.bnd_in >= 0));
        if (s.bnd_in >= 0 && q > 0) {
          const DtwStrip *below = nullptr;
          for (int e : of_strip[keys[q - 1]])
            if (strips[(size_t)e].col0 == s.col0 && strips[(size_t)e].ncol == s.ncol) below = &strips[(size_t)e];
          CHECK(below != nullptr);
          if (below) CHECK(below->row0 + below->nrows == s.row0 && below->bnd_out == s.bnd_in && below->flag_out == s.flag_in);
        }
      }
      CHECK(col == p.T);
    }
    CHECK(row == p.S);
  }
  // (the boundary arrays of different strips do not overlap)
  std::sort(bnd_ranges.begin(), bnd_ranges.end());
  for (size_t i = 1; i < bnd_ranges.size(); ++i) CHECK(bnd_ranges[i - 1].second <= bnd_ranges[i].first);

  // 5. the deadlock condition: whatever a descriptor waits on -- the kernel waits on flag_prev of a packed strip even when
  // its segment is empty -- is signalled by a strictly earlier job
  for (size_t d = 0; d < strips.size(); ++d)
    for (int f : {strips[d].flag_prev, strips[d].flag_in}) {
      CHECK(f >= -1 && f < plan.nflags);
      if (f < 0 || f >= plan.nflags) continue;
      CHECK(producer[(size_t)f] >= 0);
      if (producer[(size_t)f] >= 0) CHECK(job_of[(size_t)producer[(size_t)f]] < job_of[d]);
    }
}

static bool same(const DtwStrip &a, const DtwStrip &b) {
  return a.pair == b.pair && a.row0 == b.row0 && a.nrows == b.nrows && a.flag_in == b.flag_in && a.flag_out == b.flag_out &&
         a.bnd_in == b.bnd_in && a.bnd_out == b.bnd_out && a.col0 == b.col0 && a.ncol == b.ncol && a.flag_prev == b.flag_prev &&
         a.packed == b.packed;
}

static void check_literal(const std::vector<std::pair<int, int>> &shapes, int slots, const std::vector<DtwStrip> &strips,
                          const std::vector<int> &job_first, int nflags, int nseg, size_t ncodes, size_t nclast, size_t nbnd,
                          size_t npath) {
  std::vector<DtwPair> pairs = make_pairs(shapes, false);
  const DtwFusedPlan plan = dtw_fused_plan(pairs, 40, slots, true, false, false);
  CHECK(plan.strips.size() == strips.size());
  for (size_t i = 0; i < strips.size() && i < plan.strips.size(); ++i) CHECK(same(plan.strips[i], strips[i]));
  CHECK(plan.job_first == job_first);
  CHECK(plan.nflags == nflags && plan.nseg == nseg && !plan.any_align);
  CHECK(plan.ncodes == ncodes && plan.nclast == nclast && plan.nbnd == nbnd && plan.npath == npath);
  size_t frames = 0;
  for (const auto &s : shapes) frames += (size_t)(s.first + s.second);
  CHECK(plan.padn == frames * 40);
}

int main() {
  // fields: pair, row0, nrows, flag_in, flag_out, bnd_in, bnd_out, col0, ncol, flag_prev, packed
  context = "literal: one strip, one segment";
  check_literal({{100, 50}}, 512, {{0, 0, 100, -1, -1, -1, -1, 0, 50, -1, 0}}, {0}, 0, 1, 4 * 100, 100, 0, 50);
  // 513 rows: a two-row bottom strip (the odd remainder rounded up), packed with three empty descriptors, signals flag 0 and
  // leaves its boundary costs at 0; the 511 rows above wait for both
  context = "literal: 513 rows";
  check_literal({{513, 40}}, 512,
                {{0, 0, 2, -1, 0, -1, 0, 0, 40, -1, 1},
                 {0, 0, 0, -1, -1, -1, -1, 0, 0, -1, 1},
                 {0, 0, 0, -1, -1, -1, -1, 0, 0, -1, 1},
                 {0, 0, 0, -1, -1, -1, -1, 0, 0, -1, 1},
                 {0, 2, 511, 0, -1, 0, -1, 0, 40, -1, 0}},
                {0, 4}, 1, 1, 3 * 514, 513, 80, 40);
  // three equal pairs on two slots: two segments (ceil(6 / 2) / 2 * 1.04 = 1.56 against 2 whole and 1.8 for three), the
  // first 1.35 / 2 of the 200 columns rounded down to 128; segment 1 of every pair waits for its segment 0
  context = "literal: two segments";
  check_literal({{100, 200}, {100, 200}, {100, 200}}, 2,
                {{0, 0, 100, -1, 0, -1, -1, 0, 128, -1, 0},
                 {1, 0, 100, -1, 1, -1, -1, 0, 128, -1, 0},
                 {2, 0, 100, -1, 2, -1, -1, 0, 128, -1, 0},
                 {0, 0, 100, -1, -1, -1, -1, 128, 72, 0, 0},
                 {1, 0, 100, -1, -1, -1, -1, 128, 72, 1, 0},
                 {2, 0, 100, -1, -1, -1, -1, 128, 72, 2, 0}},
                {0, 1, 2, 3, 4, 5}, 3, 2, 3 * 13 * 100, 300, 0, 600);

  const auto batches = dtw_plan_check_batches();
  int plans = 0, segmented = 0;
  char ctx[128];
  for (size_t b = 0; b < batches.size(); ++b)
    for (int slots : {2, 8, 24, 48, 64, 512})
      for (int setting = 0; setting < 4; ++setting) {      // default, no segments, two segments at most, whole jobs first
        std::snprintf(ctx, sizeof ctx, "batch %zu, %d slots, setting %d", b + 1, slots, setting);
        context = ctx;
        const std::vector<DtwPair> pairs = make_pairs(batches[b], b % 2 == 0);
        check_plan(pairs, b == 3 ? 41 : 40, slots, setting != 1, setting == 2, setting == 3);
        ++plans;
        std::vector<DtwPair> again = pairs;
        if (dtw_fused_plan(again, 40, slots, setting != 1, setting == 2, setting == 3).nseg > 1) ++segmented;
      }
  context = "empty";
  check_plan({}, 40, 512, true, false, false);
  check_plan(make_pairs({{5, 0}, {700, 0}}, true), 40, 512, true, false, false);
  CHECK(segmented > 0);
  std::printf("dtw_plan_check: %d plans, %d of them with column segments, %d failures\n", plans, segmented, failures);
  if (failures == 0) std::printf("dtw_plan_check: ok\n");
  return failures == 0 ? 0 : 1;
}
