// estep_plan.cpp -- the launch plan of one diagonal E-step (estep_plan.hpp).  Host-only arithmetic: no HIP call, no device type.
#include "estep_plan.hpp"

#include <algorithm>

#include "../../include/vcmi.h"

namespace vcmi {

namespace {

EstepChunks chunks_of(int64_t N, int64_t len) {
  EstepChunks c;
  c.len = std::min(N, len);
  c.count = (N + c.len - 1) / c.len;
  c.last = N - (c.count - 1) * c.len;
  return c;
}
// workgroups for nfr frames in blocks of fb, at most cap
int blocks_grid(int64_t nfr, int fb, int64_t cap) { return (int)std::min<int64_t>((nfr + fb - 1) / fb, cap); }

void plan_generic(const EstepPlanInput &in, EstepPlan &p) {
  const int M = in.M, Dj = in.Dj;
  p.chunks = chunks_of(in.N, kChunk);
  const int64_t nfr[2] = {p.chunks.len, p.chunks.last};
  for (int i = 0; i < 2; ++i) {
    p.gamma_grid[i] = (int)((nfr[i] + 63) / 64);
    p.nseg[i] = (int)((nfr[i] + kSeg - 1) / kSeg);
  }
  p.stats_grid_y = (M * Dj + 255) / 256;
  p.gamma_lds = (size_t)Dj * 64 * sizeof(double);
  p.n_mu = (size_t)M * Dj;
  p.n_cst = (size_t)M;
  p.n_G = (size_t)p.chunks.len * M;
  p.n_LSE = (size_t)p.chunks.len;
  p.n_part = (size_t)p.nseg[0] * p.plen;
}

void plan_pad_odd(const EstepPlanInput &in, EstepPlan &p) {
  p.djp = in.Dj + 1;
  p.plen_p = estep_stats_len(p.djp, in.M);
  p.chunks = chunks_of(in.N, kPadChunk);
  const int64_t nfr[2] = {p.chunks.len, p.chunks.last};
  for (int i = 0; i < 2; ++i) p.pad_grid[i] = (int)std::min<int64_t>((nfr[i] * p.djp + 255) / 256, 65536);
  p.unpad_grid = (int)(((int64_t)in.M * in.Dj + 255) / 256);
  p.n_Xpad = (size_t)p.chunks.len * p.djp;
  p.n_statsp = (size_t)p.plen_p;
}

template <int DJ>
void plan_groups(const EstepPlanInput &in, EstepPlan &p) {
  using C = EstepCfg<DJ>;
  const int M = in.M, dj = in.Dj;
  const size_t wlen = (size_t)8 * C::KS * 64;
  p.ng = (M + C::MMAX - 1) / C::MMAX;
  p.Mg_last = M - (p.ng - 1) * C::MMAX;
  p.chunks = chunks_of(in.N, kGroupsChunk);
  p.prep_grid = (int)((wlen + 255) / 256);
  const int64_t nfr[2] = {p.chunks.len, p.chunks.last};
  const int Mg[2] = {C::MMAX, p.Mg_last};
  for (int i = 0; i < 2; ++i) {
    p.group_grid[i] = blocks_grid(nfr[i], C::FB, in.cus);
    p.group_reduce_grid[i] = (int)((estep_stats_len(dj, Mg[i]) + 255) / 256);
  }
  p.body_lds = C::LDS_BYTES;
  p.n_raw = (size_t)M * (1 + 2 * dj);
  p.n_Wpack = wlen * p.ng;
  p.n_cinit = (size_t)C::MMAX * p.ng;
  p.n_refiv = (size_t)M * dj;
  p.n_refc = (size_t)2 * M;
  p.n_G = (size_t)p.ng * p.chunks.len * C::MMAX;
  p.n_LSE = (size_t)p.ng * p.chunks.len + kCombineGrid;
  p.n_part = (size_t)in.cus * ((size_t)C::MMAX * (1 + 2 * dj) + 1);
}

// grid, rows of partial statistics and LDS bytes of one FP64 launch of `body` (not kBodySplit) over nfr frames
template <int DJ>
void soft_launch(EstepBody body, int64_t nfr, int cus, int wpt, int *grid, int *rows, size_t *lds) {
  if constexpr (!EstepCfg<DJ>::SPLIT) {
    if (body == kBodySmall1 || body == kBodySmall2) {
      using S1 = EstepSmallCfg<DJ, 1>;
      using S2 = EstepSmallCfg<DJ, 2>;
      const bool one = body == kBodySmall1;
      *grid = blocks_grid(nfr, one ? S1::FB : S2::FB, (int64_t)cus * (one ? S1::WG_PER_CU : S2::WG_PER_CU));
      *rows = *grid * 2;
      *lds = one ? S1::LDS_BYTES : S2::LDS_BYTES;
      return;
    }
    if (body == kBodyWave) {
      *grid = blocks_grid(nfr, EstepWaveCfg<DJ>::FB, cus);
      *rows = *grid;
      *lds = EstepWaveCfg<DJ>::LDS_BYTES;
      return;
    }
  }
  *grid = blocks_grid(nfr, EstepCfg<DJ>::FB, cus);
  *rows = *grid * wpt;
  *lds = EstepCfg<DJ>::LDS_BYTES;
}

template <int DJ>
void plan_hard(const EstepPlanInput &in, EstepPlan &p) {
  using CH = EstepHardCfg<DJ>;
  const int64_t N = in.N;
  const int M = in.M, dj = in.Dj, cus = in.cus;
  p.sample = in.path == VCMI_ESTEP_AUTO;
  p.MT = (M + 15) / 16;
  p.MK = M + 1;
  p.nchunks = (N + kHardChunk - 1) / kHardChunk;
  p.nsample = std::min<int64_t>(16, p.nchunks);
  p.cstride = p.nchunks / p.nsample;
  p.npmax = (N + kHardPiece - 1) / kHardPiece + M;
  p.prow = 2 * (int64_t)dj + 2;
  p.hprep_grid = (p.MT * CH::NI * 64 + 255) / 256 + 4 * p.MT;
  p.sample_grid = (int)(p.nsample * kHardSamplePasses);
  p.key_grid = (int)std::min<int64_t>(p.nchunks, cus);
  p.scan_grid = p.MK;
  p.scatter_grid = (int)p.nchunks;
  p.hstats_grid = (int)p.npmax;
  p.hreduce_grid = M;
  p.gather_grid = cus * 4;
  p.key_lds = CH::lds_bytes(p.MT) + (size_t)p.MK * sizeof(int);
  p.scatter_lds = (size_t)17 * p.MK * sizeof(int);
  // the gathered soft frames: their number is the device's, the grid covers the CUs; then (sample) every frame
  soft_launch<DJ>(p.soft_body, (int64_t)1 << 40, cus, p.wpt, &p.gathered_grid, &p.gathered_rows, &p.soft_lds);
  if (p.sample) soft_launch<DJ>(p.soft_body, N, cus, p.wpt, &p.allsoft_grid, &p.allsoft_rows, &p.soft_lds);
  p.n_Xsoft = (size_t)N * dj;
  p.n_W16 = (size_t)p.MT * CH::TILE_BYTES;
  p.n_probe = (size_t)p.nsample * kHardSamplePasses * p.MK;
  p.n_ctl = (size_t)kCtlLen;
  p.n_hkeys = (size_t)2 * N + (size_t)(p.nchunks + 1) * p.MK;
  p.n_hpart = (size_t)p.npmax * p.prow;
  p.n_hllm = (size_t)M;
}

template <int DJ>
void plan_mfma(const EstepPlanInput &in, EstepPlan &p) {
  using C = EstepCfg<DJ>;
  const int64_t N = in.N;
  const int M = in.M, dj = in.Dj, cus = in.cus;
  p.mtp = 1;
  while (16 * p.mtp < M) p.mtp *= 2;
  p.wpt = 8 / p.mtp;
  p.share = p.mtp < 8;
  p.prep_grid = (8 * C::KS * 64 + 255) / 256;
  p.n_raw = (size_t)M * (1 + 2 * dj);
  p.n_Wpack = (size_t)8 * C::KS * 64;
  p.n_cinit = (size_t)C::MMAX;
  p.n_refiv = (size_t)M * dj;
  p.n_refc = (size_t)2 * M;
  // the partial rows of estep_mfma_kernel over all N frames, whatever the body: what every call of the shape has reserved
  int rows_max = blocks_grid(N, C::FB, cus) * p.wpt;
  if constexpr (C::SPLIT) {
    p.body = kBodySplit;
    p.body_lds = C::LDS_BYTES;
    p.chunks = chunks_of(N, kSplitChunk);
    const int64_t nfr[2] = {p.chunks.len, p.chunks.last};
    for (int i = 0; i < 2; ++i) {
      p.body_grid[i] = blocks_grid(nfr[i], C::FB, cus);
      p.body_rows[i] = p.body_grid[i] * p.wpt;
    }
    p.n_G = (size_t)p.chunks.len * C::MMAX;
  } else {
    p.chunks = chunks_of(N, N);
    const bool small = M <= 32 && !in.no_small;
    p.soft_body = !small ? kBodyOne : M <= 16 ? kBodySmall1 : kBodySmall2;
    p.body = (p.mtp == 8 && in.wave_kernel) ? kBodyWave : p.soft_body;
    soft_launch<DJ>(p.body, N, cus, p.wpt, &p.body_grid[0], &p.body_rows[0], &p.body_lds);
    p.body_grid[1] = p.body_grid[0];
    p.body_rows[1] = p.body_rows[0];
    // Frames that one mixture owns never see an FP64 MFMA (estep_hard.hpp) -- where there are enough frames to pay for the
    // screen, the thread has not pinned the one-kernel path, and the model has more than one mixture tile: estep_small_kernel
    // takes 0.30 ms per 1.25e6 frames whatever the data, the hard-assignment chain 0.42 where every frame has an owner
    // (vcmi_estep_set_path(VCMI_ESTEP_HARD) still takes it)
    const int path = in.no_hard ? VCMI_ESTEP_SOFT : in.path;
    p.hard = N >= kHardMinFrames && N < ((int64_t)1 << 31) && M <= kHardMaxM && path != VCMI_ESTEP_SOFT;
    if (path == VCMI_ESTEP_AUTO && M <= 16 && !in.no_small) p.hard = false;
    if (p.hard) {
      plan_hard<DJ>(in, p);
      rows_max = std::max(rows_max, std::max(p.gathered_rows, p.allsoft_rows));
    }
    // (a hard chain that the launcher has to demote runs the body)
    rows_max = std::max(rows_max, p.body_rows[0]);
  }
  p.n_part = (size_t)rows_max * p.plen;
}

}  // namespace

EstepPlan estep_plan(const EstepPlanInput &in) {
  EstepPlan p;
  p.plen = estep_stats_len(in.Dj, in.M);
  p.reduce_grid = (int)((p.plen + 63) / 64);
  p.copy_down = in.device_block && !estep_mfma_shape(in.Dj, in.M, in.generic);
  if (mfma_dims(in.Dj, in.generic)) {
    p.route = estep_mfma_shape(in.Dj, in.M, in.generic) ? kRouteMfma : kRouteGroups;
    p.DJ = estep_mfma_dj(in.Dj);
    with_mfma_dj(in.Dj, [&](auto dj_c) -> int {
      constexpr int DJ = decltype(dj_c)::value;
      if (p.route == kRouteMfma) plan_mfma<DJ>(in, p);
      else plan_groups<DJ>(in, p);
      return 0;
    });
  } else if (mfma_dims(in.Dj + 1, in.generic)) {
    p.route = kRoutePadOdd;
    plan_pad_odd(in, p);
  } else {
    p.route = kRouteGeneric;
    plan_generic(in, p);
  }
  return p;
}

}  // namespace vcmi
