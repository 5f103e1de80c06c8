// dtw_plan.cpp -- see dtw_plan.hpp.  Host arithmetic only.
#include "dtw_plan.hpp"

#include <algorithm>
#include <cmath>

namespace vcmi {

DtwFusedPlan dtw_fused_plan(std::vector<DtwPair> &pairs, int row_len, int slots, bool segments_allowed, bool two_segments_max,
                            bool whole_first) {
  const int n = (int)pairs.size();
  const int dmax = row_len;
  // single-strip pairs largest first (shortens the tail); the strips of long templates are ordered by level: all
  // bottom strips lead the grid -- they are what the upper strips wait for -- and the upper strips follow the
  // single-strip pairs, by which time their predecessors are done.
  std::stable_sort(pairs.begin(), pairs.end(), [](const DtwPair &a, const DtwPair &b) {
    return (int64_t)a.S * a.T > (int64_t)b.S * b.T;
  });
  size_t ncodes = 0, nclast = 0, nbnd = 0, padn = 0, npath = 0;
  bool any_align = false;
  int nflags = 0;
  // pass 1: the row strips of every pair, whole-length (col0 = 0, ncol = T): one-wave or wider bottom strips of long
  // templates (levels[0]), single-strip pairs, the strips above by level.
  std::vector<std::vector<DtwStrip>> levels;
  std::vector<DtwStrip> singles;
  for (int k = 0; k < n; ++k) {
    DtwPair &p = pairs[k];
    const int Se = (p.S + 1) & ~1;
    p.fcodes_off = (int64_t)ncodes;
    ncodes += (size_t)((p.T + 15) >> 4) * Se;
    p.clast_off = (int64_t)nclast;
    nclast += (size_t)p.S;
    p.path32_off = (int64_t)npath;
    npath += (size_t)p.T;
    any_align = any_align || p.newtgt != nullptr;
    p.spad_off = (int64_t)padn;
    padn += (size_t)p.T * dmax;
    p.tpad_off = (int64_t)padn;
    padn += (size_t)p.S * dmax;
    if (p.T == 0) continue;
    const int nstr = (p.S + kFusedRows - 1) / kFusedRows;
    if (nstr == 1) {
      singles.push_back(DtwStrip{k, 0, p.S, -1, -1, -1, -1, 0, p.T, -1, 0});
      continue;
    }
    int first = p.S - kFusedRows * (nstr - 1);      // remainder strip at the bottom, an even number of rows
    first += first & 1;
    int row = 0;
    for (int s = 0; s < nstr; ++s) {
      const int rows = (s == 0) ? first : std::min(kFusedRows, p.S - row);
      DtwStrip ds{k, row, rows, -1, -1, -1, -1, 0, p.T, -1, 0};
      if (s > 0) ds.bnd_in = (int64_t)(nbnd - (size_t)2 * p.T);
      if (s + 1 < nstr) {
        ds.bnd_out = (int64_t)nbnd;
        nbnd += (size_t)2 * p.T;
      }
      if ((int)levels.size() <= s) levels.resize(s + 1);
      levels[s].push_back(ds);
      row += rows;
    }
  }
  // Column segments.  The jobs of a batch take about the same time (T columns each), so with one whole-length job per
  // workgroup a slot runs a whole number of them and the batch takes ceil(jobs / slots) job times: 1093 jobs on 512 slots
  // = 3, for 2.13 job times of work.  Cutting every strip's columns into `nseg` segments (a segment starts from the last
  // cost column its predecessor left in clast_ws) makes the unit smaller: 5 x 1093 jobs = 10.7 fifth-rounds.  A 100-column
  // segment costs what a 100-column sequence costs (7k cycles of prologue + 2.3k per column, cycle counter) PROVIDED the
  // jobs synchronise without agent-scope fences (see dtw_wait_flag): with one acquire / release pair per job the same
  // segment took 350k cycles instead of 250k and segments did not pay (1.72 / 1.68 / 1.74 / 1.82 / 2.43 ms for nseg = 1 / 2
  // / 3 / 4 / 8) -- which an earlier revision of this comment blamed on workgroup dispatch.  Now 1.69 / 1.52 / 1.50 / 1.51 /
  // 1.49 / 1.50 / 1.52 / 1.57 ms for nseg = 1 / 2 / 3 / 4 / 5 / 6 / 8 / 10.  nseg minimises ceil(jobs / slots) / nseg with 4 % per
  // extra segment -- its prologue, and above all its TRAFFIC: every segment job loads its strip's template rows again, 0.1 GB
  // per 1000 pairs and segment (0.39 GB at nseg = 1, 0.78 GB at nseg = 5, against 0.32 GB algorithmic), while the measured
  // times are flat from nseg = 2 to 8, so fewer is better (3 for the benchmark batch) --, segments of at least 64 columns,
  // nothing cut when everything fits one round.  The
  // segments are drawn from a ticket counter by persistent workgroups, one per slot (dtw_fused_persistent_kernel: 1.49 ms
  // against 1.53 ms with one workgroup per job in grid order at D = 40; the D = 48 kernel, whose persistent form spills 16
  // registers, stays with grid order: 1.77 against 1.80 ms).
  std::vector<DtwStrip> packed, wide;
  if (!levels.empty())
    for (const DtwStrip &ds : levels[0]) (ds.nrows <= 128 ? packed : wide).push_back(ds);
  size_t nwhole = wide.size() + singles.size();
  for (size_t l = 1; l < levels.size(); ++l) nwhole += levels[l].size();
  int nseg = 1;
  {
    int64_t tsum = 0, tcnt = 0;
    for (const DtwPair &p : pairs)
      if (p.T > 0) {
        tsum += p.T;
        ++tcnt;
      }
    const int tavg = (int)(tsum / std::max<int64_t>(tcnt, 1));
    const double base_jobs = (double)((packed.size() + 3) / 4) + (double)nwhole;
    double best = 1e30;
    for (int c : {1, 2, 3, 4, 5, 6, 8}) {
      if (c > 1 && (!segments_allowed || tavg / c < 64 || base_jobs <= slots)) break;
      if (c > 2 && two_segments_max) break;
      const double t = std::ceil(base_jobs * c / slots) / c * (1.0 + 0.04 * (c - 1));
      if (t < best - 1e-9) {
        best = t;
        nseg = c;
      }
    }
  }
  // pass 2: job order, segment by segment: packed groups of one-wave bottom strips (four per workgroup, padded with empty
  // strips), the other bottom strips, the single-strip pairs (largest first), the upper strips level by level.  A job
  // waits only for jobs earlier in the order: the strip below (same segment) and its own previous segment.
  while (packed.size() % 4) packed.push_back(DtwStrip{packed.empty() ? 0 : packed.back().pair, 0, 0, -1, -1, -1, -1, 0, 0, -1, 0});
  std::vector<DtwStrip> whole = wide;
  whole.insert(whole.end(), singles.begin(), singles.end());
  for (size_t l = 1; l < levels.size(); ++l) whole.insert(whole.end(), levels[l].begin(), levels[l].end());
  // Segments of DECREASING length: the jobs drawn last decide how long slots idle at the end of the kernel (on average half
  // a job), so segment j gets the weight 1 + beta (nseg - 1 - 2 j) / (nseg - 1) -- 1.35 : 1 : 0.65 for three.  Measured at
  // beta = 0 / 0.2 / 0.3 / 0.4 / 0.5 / 0.6: 1.46 / 1.45 / 1.43 / 1.43 / 1.45 / 1.44 ms (D = 41: 1.59 -> 1.54).
  constexpr double seg_beta = 0.35;
  auto seg_bounds = [&](int T, int k) {            // first column of segment k (multiples of 16), k = nseg -> T
    if (k >= nseg) return T;
    if (k <= 0) return 0;
    double acc = 0.0;
    for (int j = 0; j < k; ++j) acc += 1.0 + (nseg > 1 ? seg_beta * (nseg - 1 - 2 * j) / (nseg - 1) : 0.0);
    return (int)(T * acc / nseg) & ~15;
  };
  // the strip below every upper strip: a packed bottom or a whole-length strip of the same pair that ends where it starts
  std::vector<int> below(whole.size(), -1);
  std::vector<char> below_packed(whole.size(), 0);
  {
    std::vector<std::vector<int>> by_pair_packed((size_t)n), by_pair_whole((size_t)n);
    for (size_t i = 0; i < packed.size(); ++i)
      if (packed[i].nrows > 0) by_pair_packed[(size_t)packed[i].pair].push_back((int)i);
    for (size_t i = 0; i < whole.size(); ++i) by_pair_whole[(size_t)whole[i].pair].push_back((int)i);
    for (size_t i = 0; i < whole.size(); ++i) {
      const DtwStrip &ds = whole[i];
      if (ds.bnd_in < 0) continue;
      for (int j : by_pair_packed[(size_t)ds.pair])
        if (packed[(size_t)j].row0 + packed[(size_t)j].nrows == ds.row0) {
          below[i] = j;
          below_packed[i] = 1;
        }
      for (int j : by_pair_whole[(size_t)ds.pair])
        if (whole[(size_t)j].row0 + whole[(size_t)j].nrows == ds.row0) below[i] = j;
    }
  }
  // Round 4 experiment (off by default: `vcmi_debug_force` kDbgDtwWholeFirst): whole-length jobs for the first rounds,
  // segments only where they balance.  Cutting EVERY strip makes every strip's template rows travel nseg times (2.7 x the
  // algorithmic bytes at nseg = 3), and the segments earn their keep in the last round only: with J jobs on S slots the first
  // floor(J / S) - 1 rounds are full whatever the unit is.  So that many slots' worth of single-strip pairs ran as ONE job
  // each, ahead of everything else, and only the rest was cut -- the same number of (1 / nseg)-rounds on paper, a third of
  // the re-reads (2.06 template loads per strip instead of 3: 1.55 x the algorithmic bytes).  Measured, 1000 pairs, one box,
  // alternating: 1.455 / 1.477 ms against 1.419 / 1.424 ms with every strip cut (two segments at most: 1.515): the long jobs
  // of the first round end ragged, and the slots that finish early find only segments whose predecessors are still running.
  // The re-reads are what the balance costs; every strip stays cut.
  std::vector<char> run_whole(whole.size(), 0);
  if (nseg > 1 && whole_first) {
    const double base_jobs = (double)(packed.size() / 4) + (double)whole.size();
    int64_t quota = (int64_t)slots * std::max<int64_t>(0, (int64_t)std::floor(base_jobs / slots) - 1);
    for (size_t i = wide.size(); i < wide.size() + singles.size() && quota > 0; ++i, --quota) run_whole[i] = 1;
  }
  std::vector<std::vector<int>> pflag(packed.size(), std::vector<int>((size_t)nseg, -1));
  std::vector<std::vector<int>> wflag(whole.size(), std::vector<int>((size_t)nseg, -1));
  DtwFusedPlan plan;
  std::vector<DtwStrip> &strips = plan.strips;
  std::vector<int> &job_first = plan.job_first;
  auto segment_of = [&](DtwStrip ds, int k, std::vector<int> &flags_of, bool has_consumer_above) {
    const int T = ds.nrows > 0 ? pairs[(size_t)ds.pair].T : 0;
    ds.col0 = seg_bounds(T, k);
    ds.ncol = std::max(0, seg_bounds(T, k + 1) - ds.col0);
    ds.flag_prev = -1;
    for (int kp = k - 1; kp >= 0 && ds.flag_prev < 0; --kp) ds.flag_prev = flags_of[(size_t)kp];
    if (ds.ncol > 0 && (has_consumer_above || seg_bounds(T, k + 1) < T)) flags_of[(size_t)k] = ds.flag_out = nflags++;
    return ds;
  };
  for (int k = 0; k < nseg; ++k) {
    for (size_t i = 0; i + 3 < packed.size(); i += 4) {
      bool any = false;
      DtwStrip g4[4];
      for (int q = 0; q < 4; ++q) {
        g4[q] = segment_of(packed[i + q], k, pflag[i + q], packed[i + q].bnd_out >= 0);
        g4[q].packed = 1;
        any = any || g4[q].ncol > 0;
      }
      if (!any) continue;
      job_first.push_back((int)strips.size());
      strips.insert(strips.end(), g4, g4 + 4);
    }
    for (size_t i = 0; i < whole.size(); ++i) {
      DtwStrip ds = segment_of(whole[i], k, wflag[i], whole[i].bnd_out >= 0);
      if (run_whole[i]) {                          // one job over all columns, in the first pass
        if (k > 0) continue;
        ds = whole[i];
        ds.col0 = 0;
        ds.ncol = pairs[(size_t)ds.pair].T;
        ds.flag_prev = ds.flag_in = ds.flag_out = -1;      // a single strip: nobody waits for it, it waits for nobody
      }
      if (ds.ncol <= 0) continue;                  // (short sequences: fewer segments than nseg)
      // (the strip below has the same T, hence the same segment boundaries: its segment k exists whenever this one does)
      if (below[i] >= 0) ds.flag_in = below_packed[i] ? pflag[(size_t)below[i]][(size_t)k] : wflag[(size_t)below[i]][(size_t)k];
      job_first.push_back((int)strips.size());
      strips.push_back(ds);
    }
  }
  plan.nflags = nflags;
  plan.nseg = nseg;
  plan.any_align = any_align;
  plan.ncodes = ncodes;
  plan.nclast = nclast;
  plan.nbnd = nbnd;
  plan.padn = padn;
  plan.npath = npath;
  return plan;
}

}  // namespace vcmi
