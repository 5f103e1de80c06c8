// estep.hip -- E-step of EM for a diagonal-covariance GMM on joint features, MI355X (gfx950).
//
// Call site in the reference: bin/train_gmm.jl:103 `gmm[:fit](dataset.X')` (scikit-learn through PyCall); the
// joint feature matrix is built by src/datasets.jl:52-77.  The arithmetic itself is third-party (sklearn.mixture);
// what is implemented here is its published definition:
//   l_nm = log w_m - (Dj log 2pi + sum_d log var_md + sum_d (x_nd - mu_md)^2 / var_md) / 2
//   lse_n = logsumexp_m l_nm,   gamma_nm = exp(l_nm - lse_n)
//   S0_m = sum_n gamma_nm,  S1_md = sum_n gamma_nm x_nd,  S2_md = sum_n gamma_nm x_nd^2,  loglik = sum_n lse_n
// Output buffer layout (device): [S0 (M) | S1 (Dj,M) | S2 (Dj,M) | loglik] -- contiguous so that the multi-GPU
// path is ONE all-reduce(sum) of M(1+2Dj)+1 doubles over RCCL.
//
// This file is the host side: scratch, the launchers and the entry points.  WHAT a call launches is decided by the host-only
// plan (estep_plan.cpp, checked on the CPU); the kernels live in headers of this translation unit, which needs the AGPR half
// of the register file (csrc/Makefile):
//  * estep_mfma.hpp   estep_mfma_kernel (v_mfma_f64_16x16x4_f64), instantiated for DJ = 32, 48, 64, 80 (one kernel) and 112,
//                     160 (two kernels, gamma through HBM), M <= 128: both the log-density  l = [x^2, x] . [-iv/2 ; mu iv] + c
//                     and the statistics  gamma' [x, x^2]  are dense FP64 contractions.  A workgroup of 8 waves owns a strided
//                     set of frame blocks; a wave owns 16 mixtures, whose weight fragments and statistics accumulators stay in
//                     registers for the whole kernel.  Per-workgroup partial statistics are reduced in a fixed order by a
//                     second kernel, so results are bit-identical run to run (no FP64 atomics).  More than 128 mixtures run
//                     as groups of 128.
//  * estep_small.hpp  estep_small_kernel: M <= 32 (one or two mixture tiles), DJ <= 80 -- workgroups as small as the model.
//  * estep_hard.hpp, estep_path.hpp  the hard-assignment chain (N >= 65536, DJ <= 80): frames that one mixture owns are
//                     settled by a certified bf16 screen and summed without an FP64 MFMA, the rest is gathered and goes
//                     through the kernels above; which of the two a call takes is decided on the device from a sample of
//                     its own frames.
//  * estep_wave.hpp   estep_wave_kernel: the one-barrier-per-block experiment (test hook, M > 64).
//  * estep_generic.hpp  the generic kernels (any Dj, M: gamma to an HBM workspace in chunks, then per-(m,d) sequential
//                     accumulation over fixed frame segments), the fixed-order reduction, the group and padding kernels.
//  * estep_operands.hpp  parameters -> MFMA operands: the pinned staging ring, the copy kernel, estep_prep_kernel.
#include "estep_internal.hpp"
#include "estep_plan.hpp"
#include "devgroup.hpp"
#include "hostpipe.hpp"
#define VCMI_DPP_NO_COPY 1           // (fp64_exp.hpp: lane permutations without the copy of the old value)
#include "fp64_exp.hpp"
#ifndef VCMI_ESTEP_EXP_SKIP
#define VCMI_ESTEP_EXP_SKIP 1      // wave-uniform skip of the softmax exps of slot groups that are hopeless for the four frames of a pass (A/B: -0.9 %)
#endif

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace vcmi {
static constexpr double kLog2Pi = 1.8378770664093454835606594728112;
typedef double d4 __attribute__((ext_vector_type(4)));
}  // namespace vcmi
#include "estep_generic.hpp"
#include "estep_mfma.hpp"
#include "estep_wave.hpp"
#include "estep_small.hpp"
#include "estep_hard.hpp"
#include "estep_path.hpp"
#include "estep_operands.hpp"
namespace vcmi {

// ------------------------------------------------------------------------------------------------
// scratch of the calling thread
// ------------------------------------------------------------------------------------------------
struct EstepScratch {
  DevBuf<double> mu, iv, cst, G, LSE, part, Wpack, cinit, raw, refiv, refc, Xpad, statsp;
  DevBuf<unsigned long long> mfma_count;      // optional measurement counter (vcmi_debug_estep_mfma); null: the kernels count nothing
  // the hard-assignment path (estep_hard.hpp, estep_path.hpp): operands, the sample's histograms, the path control words, sort
  // scratch, pieces and the soft frames' matrix
  DevBuf<unsigned char> W16;
  DevBuf<int> probe;                           // sample histograms (16 x (M + 1))
  DevBuf<int64_t> ctl;                         // kCtlLen control words (estep_cfg.hpp)
  DevBuf<int> hkeys;                           // key (N) | perm (N) | chunkhist (nchunks x (M + 1)) | total (M + 1)
  DevBuf<double> hpart, hllm, Xsoft;
  bool last_hard = false;                      // the last diagonal E-step of this thread launched the hard-assignment path's kernels
  EstepStaging stage;
  std::vector<double> hblock;                  // estep_device_block: the host copy of a device parameter block
  StreamOrder order;   // calls of one thread on different streams share the buffers above
};
static EstepScratch &scratch() {
  static thread_local EstepScratch s;
  return s;
}
// vcmi_estep_set_path: which of the two paths the diagonal E-step of this host thread takes (default: decided per call, from
// the call's own data)
static int &estep_path_choice_ref() {
  static thread_local int p = VCMI_ESTEP_AUTO;
  return p;
}

void estep_reduce_launch(const double *part, int nrows, int64_t plen, double *stats, hipStream_t st, int accumulate, const int64_t *only_if) {
  hipLaunchKernelGGL(estep_reduce_kernel, dim3((unsigned)((plen + 63) / 64)), dim3(256), 0, st, part, nrows, plen, stats, accumulate, only_if);
}
void estep_sum_launch(const double *v, int64_t n, double *out, hipStream_t st) {
  hipLaunchKernelGGL(estep_sum_kernel, dim3(1), dim3(256), 0, st, v, n, out);
}

// ------------------------------------------------------------------------------------------------
// the plan of a call, and what every launcher is handed
// ------------------------------------------------------------------------------------------------
// The input of estep_plan for a call of this thread on the current device.  The CU count is asked for once per call, and
// only where a route reads it.
static EstepPlanInput estep_plan_input(int64_t N, int Dj, int M, bool device_block) {
  EstepPlanInput in;
  in.N = N;
  in.Dj = Dj;
  in.M = M;
  in.path = estep_path_choice_ref();
  in.generic = debug_flag(kDbgEstepGeneric);
  in.no_small = debug_flag(kDbgEstepNoSmall);
  in.no_hard = debug_flag(kDbgEstepNoHard);
  in.wave_kernel = debug_flag(kDbgEstepWaveKernel);
  in.device_block = device_block;
  if (N > 0 && (mfma_dims(Dj, in.generic) || mfma_dims(Dj + 1, in.generic))) {
    int dev = 0;
    in.cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&in.cus, hipDeviceAttributeMultiprocessorCount, dev);
  }
  return in;
}

// Where a call's model parameters are: three host arrays, or one DEVICE block [w (M) | mu (dj,M) | var (dj,M)] that the caller
// keeps alive and orders on the call's stream (vcmi_gmm_em_diag: the M-step kernel wrote it).
struct EstepParams {
  const double *w = nullptr, *mu = nullptr, *var = nullptr, *block = nullptr;
  static EstepParams host(const double *w, const double *mu, const double *var) { return {w, mu, var, nullptr}; }
  static EstepParams device(const double *block) { return {nullptr, nullptr, nullptr, block}; }
};
// One E-step of the MFMA kernels: N frames at dX (dj doubles each) -> dstats on st; draw: the parameters on the device,
// [w (M) | mu (dj,M) | var (dj,M)] (estep_operands)
struct EstepCall {
  const double *dX;
  int64_t N;
  int dj, M;
  double *dstats;
  hipStream_t st;
  const double *draw;
  // the means of the exact re-evaluation are the uploaded parameters themselves
  const double *dmu() const { return draw + M; }
};

// every reservation of the plan but the hard chain's (estep_hard_launch: a chain that is demoted reserves nothing) and the
// staging slots (estep_stage_params)
static int estep_reserve(EstepScratch &sc, const EstepPlan &p) {
  VCMI_TRY(sc.Wpack.reserve(p.n_Wpack));
  VCMI_TRY(sc.cinit.reserve(p.n_cinit));
  VCMI_TRY(sc.refiv.reserve(p.n_refiv));
  VCMI_TRY(sc.refc.reserve(p.n_refc));
  VCMI_TRY(sc.mu.reserve(p.n_mu));
  VCMI_TRY(sc.iv.reserve(p.n_mu));
  VCMI_TRY(sc.cst.reserve(p.n_cst));
  VCMI_TRY(sc.Xpad.reserve(p.n_Xpad));
  VCMI_TRY(sc.statsp.reserve(p.n_statsp));
  VCMI_TRY(sc.G.reserve(p.n_G));
  VCMI_TRY(sc.LSE.reserve(p.n_LSE));
  VCMI_TRY(sc.part.reserve(p.n_part));
  return VCMI_OK;
}

// One block of n parameters through the ring: fill(h) writes the next pinned slot, the copy kernel takes it to the slot's own
// device copy -> *dblock.  The host waits only for the copy that last used the slot (eight calls ago).
template <class Fill>
static int estep_stage_params(EstepScratch &sc, size_t n, hipStream_t st, const Fill &fill, const double **dblock) {
  VCMI_TRY(sc.raw.reserve(EstepStaging::kSlots * n));    // one device copy per staging buffer
  VCMI_TRY(sc.stage.reserve(n));
  const int b = sc.stage.next;
  sc.stage.next = (sc.stage.next + 1) % EstepStaging::kSlots;
  VCMI_HIP(hipEventSynchronize(sc.stage.copied[b]));
  double *h = sc.stage.host[b], *dslot = sc.raw.p + (size_t)b * n;
  fill(h);
  // (a copy kernel reading the pinned slot, not hipMemcpyAsync: the copy engine's hand-over to the compute queue costs
  // ~20 us of idle GPU per call, a kernel on the same queue a few.  Round 4 let the prep kernel read the pinned slot itself
  // and write the device copy -- one launch less -- and lost 7 us per call: its threads read every parameter three or four
  // times, across the link.)
  hipLaunchKernelGGL(estep_param_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h, dslot, n);
  VCMI_HIP(hipEventRecord(sc.stage.copied[b], st));
  *dblock = dslot;
  return VCMI_OK;
}

// ------------------------------------------------------------------------------------------------
// kRouteMfma: operands, then one launcher per body
// ------------------------------------------------------------------------------------------------
// Scratch, the parameters on the device (host arrays: staged through the pinned ring; a device block is read where it is: no
// staging slot, no copies, no event, nothing the host waits for) and the prep kernel.  Everything from the prep kernel on is
// the same code on the same operands: the same parameter values give the same bits from either source.
template <int DJ>
static int estep_operands(EstepScratch &sc, const EstepPlan &p, const EstepParams &prm, int dj, int M, hipStream_t st, const double **draw) {
  VCMI_TRY(estep_reserve(sc, p));
  *draw = prm.block;
  if (!*draw)
    VCMI_TRY(estep_stage_params(sc, p.n_raw, st, [&](double *h) {
      memcpy(h, prm.w, sizeof(double) * M);
      memcpy(h + M, prm.mu, sizeof(double) * M * dj);
      memcpy(h + M + (size_t)M * dj, prm.var, sizeof(double) * M * dj);
    }, draw));
  hipLaunchKernelGGL(estep_prep_kernel<DJ>, dim3(p.prep_grid), dim3(256), 0, st, *draw, M, dj, sc.Wpack.p, sc.cinit.p, sc.refiv.p, sc.refc.p);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// One FP64 launch of `body` (kBodySmall1 / kBodySmall2 / kBodyOne; DJ <= 80) over the nfr frames at Xp -- their number read
// from *ndev on the device where that is given -- + the fixed-order reduction of its `rows` partial rows into dstats.
template <int DJ>
static int estep_soft_launch(EstepScratch &sc, const EstepPlan &p, const EstepCall &c, EstepBody body, int grid, int rows,
                             const double *Xp, int64_t nfr, const int64_t *ndev, int accumulate) {
  using C = EstepCfg<DJ>;
  auto small = [&](auto cfg, auto kern) -> int {
    using CS = decltype(cfg);
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CS::LDS_BYTES));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * CS::NW), CS::LDS_BYTES, c.st, Xp, nfr, c.M, sc.Wpack.p, sc.cinit.p, sc.part.p, p.plen,
                       c.dmu(), sc.refiv.p, sc.refc.p, c.dj, sc.mfma_count.p, ndev);
    return VCMI_OK;
  };
  if (body == kBodySmall1) {
    VCMI_TRY(small(EstepSmallCfg<DJ, 1>{}, estep_small_kernel<DJ, 1>));
  } else if (body == kBodySmall2) {
    VCMI_TRY(small(EstepSmallCfg<DJ, 2>{}, estep_small_kernel<DJ, 2>));
  } else {
    auto kern = p.share ? estep_mfma_kernel<DJ, 0, true> : estep_mfma_kernel<DJ, 0, false>;
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), C::LDS_BYTES, c.st, Xp, nfr, c.M, sc.Wpack.p, sc.cinit.p, sc.part.p, p.plen, c.dmu(),
                       sc.refiv.p, sc.refc.p, (double *)nullptr, c.dj, p.mtp, sc.mfma_count.p, ndev);
  }
  VCMI_HIP(hipGetLastError());
  estep_reduce_launch(sc.part.p, rows, p.plen, c.dstats, c.st, accumulate, ndev);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// The hard-assignment chain (estep_hard.hpp, estep_path.hpp): frames that one mixture owns never see an FP64 MFMA, the rest
// is gathered and goes through estep_soft_launch.  It pays where most frames have an owner and costs its pass over X on top
// of the whole one-kernel E-step where they do not (real joint mel-cepstra: DESIGN 3.3).  Decided from THIS call's data, on
// the device: the screen on a SAMPLE of 16 chunks spread over the frames (~20 us), estep_path_decide_kernel writes the
// control words, every kernel of either path starts with a look at them -- the launch sequence is fixed, nothing waits for
// the GPU, and identical inputs give identical bits whatever this thread (or any other) ran before.  vcmi_estep_set_path
// pins one.  *ran = false: nothing was launched -- the soft frames' dense matrix is as large as X in the worst case, and a
// device without room for it takes the body (the reservation used to fail the whole E-step).
template <int DJ>
static int estep_hard_launch(EstepScratch &sc, const EstepPlan &p, const EstepCall &c, bool *ran) {
  *ran = false;
  if (sc.Xsoft.reserve(p.n_Xsoft) != VCMI_OK) {
    (void)hipGetLastError();
    return VCMI_OK;
  }
  VCMI_TRY(sc.W16.reserve(p.n_W16));
  VCMI_TRY(sc.probe.reserve(p.n_probe));
  VCMI_TRY(sc.ctl.reserve(p.n_ctl));
  VCMI_TRY(sc.hkeys.reserve(p.n_hkeys));
  VCMI_TRY(sc.hpart.reserve(p.n_hpart));
  VCMI_TRY(sc.hllm.reserve(p.n_hllm));
  const int64_t N = c.N;
  const int M = c.M, dj = c.dj, MK = p.MK;
  hipStream_t st = c.st;
  int64_t *ctl = sc.ctl.p;
  const int64_t *gate = ctl + kCtlHard;
  int *key = sc.hkeys.p, *perm = key + N, *chunkhist = perm + N, *total = chunkhist + p.nchunks * MK;
  hipLaunchKernelGGL(estep_hard_prep_kernel<DJ>, dim3((unsigned)p.hprep_grid), dim3(256), 0, st, c.draw, sc.cinit.p, M, dj, sc.W16.p);
  auto kk = estep_hard_key_kernel<DJ>;
  VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.key_lds));
  if (p.sample)       // the screen on a sample of the call's frames -> the control words
    hipLaunchKernelGGL(kk, dim3((unsigned)p.sample_grid), dim3(kHardKeyThreads), p.key_lds, st, sc.W16.p, M, dj, c.dX, N, (int *)nullptr,
                       sc.probe.p, (int64_t)p.sample_grid, p.cstride, (const int64_t *)nullptr, 1);
  hipLaunchKernelGGL(estep_path_decide_kernel, dim3(1), dim3(kDecideThreads), 0, st, sc.probe.p, p.sample_grid, MK, p.sample ? -1 : 1, N, ctl);
  // The hard-assignment path proper: every kernel looks at ctl[kCtlHard] first.  (With the decision left to the device one of
  // the two chains -- these launches, or the one-kernel E-step of every frame -- returns at once, launch by launch, ~4.4 us
  // each.  Running the two chains on two streams, forked behind the decision and joined at the end, was measured in round 6:
  // the fork / join events cost more than the idle launches -- estep_fixture 0.619 against 0.608 ms, estep 0.556 against 0.526.)
  hipLaunchKernelGGL(kk, dim3((unsigned)p.key_grid), dim3(kHardKeyThreads), p.key_lds, st, sc.W16.p, M, dj, c.dX, N, key, chunkhist, p.nchunks,
                     (int64_t)1, gate, 0);
  hipLaunchKernelGGL(gmmmap_group_scan_kernel, dim3((unsigned)p.scan_grid), dim3(256), 0, st, chunkhist, p.nchunks, MK, total, gate);
  hipLaunchKernelGGL(gmmmap_group_scatter_kernel, dim3((unsigned)p.scatter_grid), dim3(256), p.scatter_lds, st, key, N, MK, chunkhist, total,
                     perm, gate);
  hipLaunchKernelGGL(estep_hard_stats_kernel<DJ>, dim3((unsigned)p.hstats_grid), dim3(256), 0, st, c.dX, dj, M, perm, total, c.dmu(), sc.refiv.p,
                     sc.hpart.p, p.prow, gate);
  hipLaunchKernelGGL(estep_hard_reduce_kernel, dim3((unsigned)p.hreduce_grid), dim3(256), 0, st, sc.hpart.p, p.prow, total, M, dj, sc.refc.p,
                     c.dstats, sc.hllm.p, gate);
  hipLaunchKernelGGL(estep_hard_ll_kernel, dim3(1), dim3(64), 0, st, sc.hllm.p, M, c.dstats, p.plen, gate);
  hipLaunchKernelGGL(estep_hard_gather_kernel, dim3((unsigned)p.gather_grid), dim3(256), 0, st, c.dX, dj, M, perm, total, sc.Xsoft.p,
                     ctl + kCtlNSoft, N, gate);
  VCMI_HIP(hipGetLastError());
  sc.last_hard = true;
  *ran = true;
  // the soft frames through the FP64 kernel, their number read on the device (the grid covers the CUs); its partials are
  // added on top ...  (both FP64 launches share the partial rows: only one of them has frames)
  VCMI_TRY(estep_soft_launch<DJ>(sc, p, c, p.soft_body, p.gathered_grid, p.gathered_rows, sc.Xsoft.p, (int64_t)1 << 40,
                                 (const int64_t *)(ctl + kCtlNSoft), /*accumulate=*/1));
  // ... or, where the sample found few owners, every frame (ctl[kCtlAllSoft] = N; 0 otherwise: both launches return at once)
  if (p.sample)
    VCMI_TRY(estep_soft_launch<DJ>(sc, p, c, p.soft_body, p.allsoft_grid, p.allsoft_rows, c.dX, N, (const int64_t *)(ctl + kCtlAllSoft),
                                   /*accumulate=*/0));
  return VCMI_OK;
}

// kBodyWave: more than 64 mixtures, every wave owns a tile of 16 -- the one-barrier-per-block kernel (estep_wave.hpp; measured
// slower than the three-barrier kernel: 1.59 against 1.32 ms -- DESIGN 3.3 round 5)
template <int DJ>
static int estep_wave_launch(EstepScratch &sc, const EstepPlan &p, const EstepCall &c) {
  using CW = EstepWaveCfg<DJ>;
  auto kw = estep_wave_kernel<DJ>;
  VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kw), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CW::LDS_BYTES));
  hipLaunchKernelGGL(kw, dim3(p.body_grid[0]), dim3(512), CW::LDS_BYTES, c.st, c.dX, c.N, c.M, sc.Wpack.p, sc.cinit.p, sc.part.p, p.plen, c.dmu(),
                     sc.refiv.p, sc.refc.p, c.dj, sc.mfma_count.p);
  VCMI_HIP(hipGetLastError());
  estep_reduce_launch(sc.part.p, p.body_rows[0], p.plen, c.dstats, c.st, /*accumulate=*/0);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// kBodySplit: two kernels per chunk of frames, the responsibilities (frames x 128 doubles) through HBM in between
template <int DJ>
static int estep_split_launch(EstepScratch &sc, const EstepPlan &p, const EstepCall &c) {
  using C = EstepCfg<DJ>;
  auto kg = p.share ? estep_mfma_kernel<DJ, 1, true> : estep_mfma_kernel<DJ, 1, false>;
  auto ks = p.share ? estep_mfma_kernel<DJ, 2, true> : estep_mfma_kernel<DJ, 2, false>;
  VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kg), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES));
  VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ks), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES));
  for (int64_t i = 0; i < p.chunks.count; ++i) {
    const bool last = i == p.chunks.count - 1;
    const int64_t nfr = last ? p.chunks.last : p.chunks.len;
    const double *Xc = c.dX + i * p.chunks.len * c.dj;
    for (auto kern : {kg, ks})
      hipLaunchKernelGGL(kern, dim3(p.body_grid[last]), dim3(512), C::LDS_BYTES, c.st, Xc, nfr, c.M, sc.Wpack.p, sc.cinit.p, sc.part.p, p.plen,
                         c.dmu(), sc.refiv.p, sc.refc.p, sc.G.p, c.dj, p.mtp, sc.mfma_count.p, (const int64_t *)nullptr);
    VCMI_HIP(hipGetLastError());
    estep_reduce_launch(sc.part.p, p.body_rows[last], p.plen, c.dstats, c.st, /*accumulate=*/i > 0);
    VCMI_HIP(hipGetLastError());
  }
  return VCMI_OK;
}

// The MFMA route for one instantiated joint dimension: operands, then the body the plan names -- behind the hard-assignment
// chain where the plan wants it and the device has room.  (The first reduction overwrites dstats: no memset in front of it.)
template <int DJ>
static int estep_mfma_launch(EstepScratch &sc, const EstepPlan &p, const double *dX, int64_t N, int dj, int M, const EstepParams &prm,
                             double *dstats, hipStream_t st) {
  EstepCall c{dX, N, dj, M, dstats, st, nullptr};
  VCMI_TRY(estep_operands<DJ>(sc, p, prm, dj, M, st, &c.draw));
  sc.last_hard = false;
  if constexpr (EstepCfg<DJ>::SPLIT) {
    return estep_split_launch<DJ>(sc, p, c);
  } else {
    if (p.hard) {
      bool ran = false;
      VCMI_TRY(estep_hard_launch<DJ>(sc, p, c, &ran));
      if (ran) return VCMI_OK;
    }
    if (p.body == kBodyWave) return estep_wave_launch<DJ>(sc, p, c);
    return estep_soft_launch<DJ>(sc, p, c, p.body, p.body_grid[0], p.body_rows[0], dX, N, (const int64_t *)nullptr, /*accumulate=*/0);
  }
}

// ------------------------------------------------------------------------------------------------
// kRouteGroups
// ------------------------------------------------------------------------------------------------
// More than 128 mixtures: groups of 128, each with its own operand blocks.  Per chunk of frames: PHASE 3 per group
// (responsibilities within the group -> G_g, the group's log-sum-exp per frame), estep_group_combine_kernel (frame-wise
// log-sum-exp over the groups, rescaling of G, log-likelihood), PHASE 2 per group (statistics from G_g, partials reduced
// in fixed order into the full layout).  Every log-density within 36 nats of its group's maximum is re-evaluated term by
// term (the kernel's refinement, unconditional in PHASE 3), so mixtures that compete across two groups are exact as well.
// The parameters are HOST arrays: they are regrouped on their way into the staging slot.  Adds into dstats.
template <int DJ>
static int estep_groups_launch(EstepScratch &sc, const EstepPlan &p, const double *dX, int dj, int M, const double *w,
                               const double *mu, const double *var, double *dstats, hipStream_t st) {
  using C = EstepCfg<DJ>;
  const int ng = p.ng;
  const int64_t chunk = p.chunks.len;
  const size_t wlen = (size_t)8 * C::KS * 64;
  auto group_m = [&](int g) { return g == ng - 1 ? p.Mg_last : C::MMAX; };
  VCMI_TRY(estep_reserve(sc, p));
  const double *draw = nullptr;
  std::vector<size_t> goff((size_t)ng + 1, 0);
  VCMI_TRY(estep_stage_params(sc, p.n_raw, st, [&](double *h) {
    for (int g = 0; g < ng; ++g) {      // every group's [w | mu (dj,Mg) | var (dj,Mg)] contiguous
      const int m0 = g * C::MMAX, Mg = group_m(g);
      double *hg = h + goff[(size_t)g];
      memcpy(hg, w + m0, sizeof(double) * Mg);
      memcpy(hg + Mg, mu + (size_t)dj * m0, sizeof(double) * Mg * dj);
      memcpy(hg + Mg + (size_t)Mg * dj, var + (size_t)dj * m0, sizeof(double) * Mg * dj);
      goff[(size_t)g + 1] = goff[(size_t)g] + (size_t)Mg * (1 + 2 * dj);
    }
  }, &draw));
  for (int g = 0; g < ng; ++g) {
    const int m0 = g * C::MMAX;
    hipLaunchKernelGGL(estep_prep_kernel<DJ>, dim3((unsigned)p.prep_grid), dim3(256), 0, st, draw + goff[(size_t)g], group_m(g), dj,
                       sc.Wpack.p + wlen * g, sc.cinit.p + (size_t)C::MMAX * g, sc.refiv.p + (size_t)m0 * dj, sc.refc.p + 2 * m0);
  }
  VCMI_HIP(hipGetLastError());
  auto k3 = estep_mfma_kernel<DJ, 3, false>;
  auto k2 = estep_mfma_kernel<DJ, 2, false>;
  VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k3), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES));
  VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k2), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES));
  double *llpart = sc.LSE.p + (size_t)ng * chunk;
  for (int64_t i = 0; i < p.chunks.count; ++i) {
    const bool last = i == p.chunks.count - 1;
    const int64_t nfr = last ? p.chunks.last : chunk;
    const double *Xc = dX + i * chunk * dj;
    const int g2 = p.group_grid[last];
    for (int g = 0; g < ng; ++g) {
      const int m0 = g * C::MMAX, Mg = group_m(g);
      hipLaunchKernelGGL(k3, dim3(g2), dim3(512), C::LDS_BYTES, st, Xc, nfr, Mg, sc.Wpack.p + wlen * g, sc.cinit.p + (size_t)C::MMAX * g,
                         sc.LSE.p + (size_t)g * nfr, (int64_t)0, draw + goff[(size_t)g] + Mg, sc.refiv.p + (size_t)m0 * dj, sc.refc.p + 2 * m0,
                         sc.G.p + (size_t)g * chunk * C::MMAX, dj, 8, sc.mfma_count.p, (const int64_t *)nullptr);
    }
    hipLaunchKernelGGL(estep_group_combine_kernel, dim3(kCombineGrid), dim3(256), 0, st, sc.G.p, sc.LSE.p, ng, nfr, (int64_t)chunk * C::MMAX,
                       llpart);
    estep_sum_launch(llpart, (int64_t)kCombineGrid, dstats + (p.plen - 1), st);
    for (int g = 0; g < ng; ++g) {
      const int m0 = g * C::MMAX, Mg = group_m(g);
      const int64_t plen_g = estep_stats_len(dj, Mg);
      hipLaunchKernelGGL(k2, dim3(g2), dim3(512), C::LDS_BYTES, st, Xc, nfr, Mg, sc.Wpack.p, sc.cinit.p, sc.part.p, plen_g, draw, sc.refiv.p,
                         sc.refc.p, sc.G.p + (size_t)g * chunk * C::MMAX, dj, 8, sc.mfma_count.p, (const int64_t *)nullptr);
      hipLaunchKernelGGL(estep_group_reduce_kernel, dim3((unsigned)p.group_reduce_grid[g == ng - 1]), dim3(256), 0, st, sc.part.p, g2, plen_g,
                         Mg, dj, m0, M, dstats);
    }
    VCMI_HIP(hipGetLastError());
  }
  return VCMI_OK;
}

// The E-step of a plan of kRouteMfma or kRouteGroups (N > 0) -> dstats.  The groups add into dstats and regroup HOST
// parameters (a device block of such a shape was copied down: EstepPlan::copy_down).
static int estep_mfma(EstepScratch &sc, const EstepPlan &p, const double *dX, int64_t N, int Dj, int M, const EstepParams &prm, double *dstats,
                      hipStream_t st) {
  const bool groups = p.route == kRouteGroups;
  if (groups) {
    if (!prm.w) return fail(VCMI_ERR_ARG, "E-step: more than %d mixtures need host parameters", EstepCfg<80>::MMAX);
    VCMI_HIP(hipMemsetAsync(dstats, 0, p.plen * sizeof(double), st));
  }
  return with_mfma_dj(Dj, [&](auto dj_c) -> int {
    constexpr int DJ = decltype(dj_c)::value;
    return groups ? estep_groups_launch<DJ>(sc, p, dX, Dj, M, prm.w, prm.mu, prm.var, dstats, st)
                  : estep_mfma_launch<DJ>(sc, p, dX, N, Dj, M, prm, dstats, st);
  });
}

// ------------------------------------------------------------------------------------------------
// kRoutePadOdd, kRouteGeneric (dstats zeroed by the caller)
// ------------------------------------------------------------------------------------------------
// Odd joint dimension: one zero dimension more (see estep_pad_x_kernel), in chunks that bound the padded copy, each planned
// and run as an E-step of its own whose statistics are added into dstats.
static int estep_pad_odd(EstepScratch &sc, const EstepPlan &p, const EstepPlanInput &in, const double *dX, const double *w, const double *mu,
                         const double *var, double *dstats, hipStream_t st) {
  const int Dj = in.Dj, M = in.M, djp = p.djp;
  std::vector<double> mup((size_t)M * djp, 0.0), varp((size_t)M * djp, 1.0);
  for (int m = 0; m < M; ++m)
    for (int d = 0; d < Dj; ++d) {
      mup[(size_t)m * djp + d] = mu[d + (size_t)Dj * m];
      varp[(size_t)m * djp + d] = var[d + (size_t)Dj * m];
    }
  VCMI_TRY(estep_reserve(sc, p));
  EstepPlanInput inner = in;
  inner.Dj = djp;
  for (int64_t i = 0; i < p.chunks.count; ++i) {
    const bool last = i == p.chunks.count - 1;
    inner.N = last ? p.chunks.last : p.chunks.len;
    hipLaunchKernelGGL(estep_pad_x_kernel, dim3((unsigned)p.pad_grid[last]), dim3(256), 0, st, dX + i * p.chunks.len * Dj, inner.N, Dj, sc.Xpad.p);
    VCMI_TRY(estep_mfma(sc, estep_plan(inner), sc.Xpad.p, inner.N, djp, M, EstepParams::host(w, mup.data(), varp.data()), sc.statsp.p, st));
    hipLaunchKernelGGL(estep_unpad_stats_kernel, dim3((unsigned)p.unpad_grid), dim3(256), 0, st, sc.statsp.p, M, Dj, inner.N, dstats);
    VCMI_HIP(hipGetLastError());
  }
  // (mup / varp are staged into pinned memory by the inner call before it returns)
  return VCMI_OK;
}

static int estep_generic(EstepScratch &sc, const EstepPlan &p, const double *dX, int Dj, int M, const double *w, const double *mu,
                         const double *var, double *dstats, hipStream_t st) {
  std::vector<double> hmu((size_t)M * Dj), hiv((size_t)M * Dj), hc(M);
  for (int m = 0; m < M; ++m) {
    double sl = 0.0;
    for (int d = 0; d < Dj; ++d) {
      const double v = var[d + (size_t)Dj * m];
      sl += std::log(v);
      hiv[(size_t)m * Dj + d] = 1.0 / v;
      hmu[(size_t)m * Dj + d] = mu[d + (size_t)Dj * m];
    }
    hc[m] = (w[m] > 0.0 ? std::log(w[m]) : -INFINITY) - 0.5 * (Dj * kLog2Pi + sl);
  }
  const size_t shmem = p.gamma_lds;
  if (shmem > 150 * 1024) return fail(VCMI_ERR_ARG, "E-step: joint dimension %d too large", Dj);
  VCMI_TRY(estep_reserve(sc, p));
  // (through the pinned ring: hostpipe.hpp, upload_now)
  VCMI_TRY(staged_upload(sc.mu.p, hmu.data(), hmu.size() * 8, st));
  VCMI_TRY(staged_upload(sc.iv.p, hiv.data(), hiv.size() * 8, st));
  VCMI_TRY(staged_upload(sc.cst.p, hc.data(), hc.size() * 8, st));
  VCMI_HIP(hipStreamSynchronize(st));
  if (shmem > 64 * 1024)
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(estep_gamma_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  for (int64_t i = 0; i < p.chunks.count; ++i) {
    const bool last = i == p.chunks.count - 1;
    const int64_t n0 = i * p.chunks.len, nfr = last ? p.chunks.last : p.chunks.len;
    hipLaunchKernelGGL(estep_gamma_kernel, dim3((unsigned)p.gamma_grid[last]), dim3(64), shmem, st, dX, n0, nfr, Dj, M,
                       sc.mu.p, sc.iv.p, sc.cst.p, sc.G.p, sc.LSE.p);
    hipLaunchKernelGGL(estep_stats_kernel, dim3(p.nseg[last], p.stats_grid_y), dim3(256), 0, st, dX, n0, nfr, Dj, M, sc.G.p,
                       sc.LSE.p, sc.part.p, p.plen);
    estep_reduce_launch(sc.part.p, p.nseg[last], p.plen, dstats, st);
    VCMI_HIP(hipGetLastError());
  }
  return VCMI_OK;
}

// ------------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------------
// One E-step from host parameters inside the caller's StreamOrderScope (in: estep_plan_input of the call)
static int estep_run(EstepScratch &sc, const EstepPlanInput &in, const double *dX, const double *w, const double *mu, const double *var,
                     double *dstats, hipStream_t st) {
  const int64_t N = in.N;
  const int Dj = in.Dj, M = in.M;
  VCMI_TRY(estep_check_dims(N, Dj, M));
  if (!w || !mu || !var || !dstats || (N > 0 && !dX)) return fail(VCMI_ERR_ARG, "E-step: NULL argument");
  sc.last_hard = false;            // (vcmi_debug_estep_last_soft: the groups and the generic kernels never take the hard path)
  const int64_t bad = first_bad_variance(var, Dj, M);
  if (bad >= 0) return fail(VCMI_ERR_NOT_PD, "E-step: variance (%d,%d) is not positive", (int)(bad % Dj) + 1, (int)(bad / Dj) + 1);
  if (N > 0) {
    const EstepPlan p = estep_plan(in);
    if (p.route == kRouteMfma || p.route == kRouteGroups) return estep_mfma(sc, p, dX, N, Dj, M, EstepParams::host(w, mu, var), dstats, st);
    VCMI_HIP(hipMemsetAsync(dstats, 0, p.plen * sizeof(double), st));
    return p.route == kRoutePadOdd ? estep_pad_odd(sc, p, in, dX, w, mu, var, dstats, st) : estep_generic(sc, p, dX, Dj, M, w, mu, var, dstats, st);
  }
  VCMI_HIP(hipMemsetAsync(dstats, 0, estep_stats_len(Dj, M) * sizeof(double), st));
  return VCMI_OK;
}

static int estep_device(const double *dX, int64_t N, int Dj, int M, const double *w, const double *mu, const double *var,
                        double *dstats, hipStream_t st) {
  EstepScratch &sc = scratch();
  StreamOrderScope use(sc.order, st);
  VCMI_TRY(use.status());
  return estep_run(sc, estep_plan_input(N, Dj, M, /*device_block=*/false), dX, w, mu, var, dstats, st);
}

int estep_device_block(const double *dX, int64_t N, int Dj, int M, const double *dparams, double *dstats, hipStream_t st) {
  if (N == 0) {
    VCMI_HIP(hipMemsetAsync(dstats, 0, estep_stats_len(Dj, M) * sizeof(double), st));
    return VCMI_OK;
  }
  EstepScratch &sc = scratch();
  EstepPlanInput in = estep_plan_input(N, Dj, M, /*device_block=*/true);
  const EstepPlan p = estep_plan(in);
  const double *hw = nullptr;
  if (p.copy_down) {
    // odd Dj, M > 128, Dj > 160: the host code of these shapes pads, regroups or transposes the parameters
    const size_t nraw = (size_t)M * (1 + 2 * (size_t)Dj);
    sc.hblock.resize(nraw);
    VCMI_HIP(hipMemcpyAsync(sc.hblock.data(), dparams, nraw * sizeof(double), hipMemcpyDeviceToHost, st));
    VCMI_HIP(hipStreamSynchronize(st));
    hw = sc.hblock.data();
    in.device_block = false;
  }
  StreamOrderScope use(sc.order, st);
  VCMI_TRY(use.status());
  if (p.copy_down) return estep_run(sc, in, dX, hw, hw + M, hw + M + (size_t)M * Dj, dstats, st);
  sc.last_hard = false;
  return estep_mfma(sc, p, dX, N, Dj, M, EstepParams::device(dparams), dstats, st);
}

// Host-pointer E-step shared by the diagonal and the full-covariance entry points: X goes up through the pinned staging
// ring; with a device group (vcmi_set_devices) member i takes the contiguous frame block [lo, hi), computes its local
// statistics, and ONE ncclAllReduce(sum) of the packed buffer over RCCL leaves the global statistics on every member
//  -- member 0 returns them.  Two group phases, so that a member that failed never leaves the others
// waiting inside the collective.
struct EstepHostBuffers {
  DevBuf<double> X, stats;      // a member's frames and its packed statistics
};
static EstepHostBuffers &host_buffers() {      // (of the calling thread without a group, of each member's thread with one)
  static thread_local EstepHostBuffers b;
  return b;
}
int estep_host(EstepDeviceFn dev, const double *X, int64_t N, int Dj, int M, const double *w, const double *mu, const double *cov,
               int64_t plen, size_t s2len, double *S0, double *S1, double *S2, double *loglik) {
  std::vector<double> h((size_t)plen, 0.0);
  auto local = [&](int64_t lo, int64_t hi) -> int {
    EstepHostBuffers &buf = host_buffers();
    const int64_t n = hi - lo;
    VCMI_TRY(buf.X.reserve((size_t)std::max<int64_t>(n, 1) * Dj));
    VCMI_TRY(buf.stats.reserve((size_t)plen));
    if (n > 0) VCMI_TRY(staged_upload(buf.X.p, X + (size_t)lo * Dj, (size_t)n * Dj * 8, nullptr));
    VCMI_TRY(dev(buf.X.p, n, Dj, M, w, mu, cov, buf.stats.p, nullptr));
    VCMI_HIP(hipStreamSynchronize(nullptr));
    return VCMI_OK;
  };
  const int m = group_size();
  if (m == 0) {
    VCMI_TRY(check_device());
    VCMI_TRY(local(0, N));
    VCMI_HIP(hipMemcpy(h.data(), host_buffers().stats.p, (size_t)plen * 8, hipMemcpyDeviceToHost));
  } else {
    VCMI_TRY(group_run(m, [&](int i) -> int {
      int64_t lo, hi;
      shard_range(N, i, m, &lo, &hi);
      return local(lo, hi);
    }));
    VCMI_TRY(group_run(m, [&](int i) -> int {
      EstepHostBuffers &buf = host_buffers();
      VCMI_TRY(group_allreduce_sum(i, buf.stats.p, (size_t)plen, nullptr));
      if (i == 0) VCMI_HIP(hipMemcpy(h.data(), buf.stats.p, (size_t)plen * 8, hipMemcpyDeviceToHost));
      return VCMI_OK;
    }));
  }
  memcpy(S0, h.data(), sizeof(double) * M);
  memcpy(S1, h.data() + M, sizeof(double) * M * Dj);
  memcpy(S2, h.data() + M + (size_t)M * Dj, sizeof(double) * s2len);
  *loglik = h[(size_t)plen - 1];
  return VCMI_OK;
}

int estep_check_dims(int64_t N, int Dj, int M) {
  if (N < 0 || Dj < 1 || M < 1) return fail(VCMI_ERR_DIM, "E-step: N=%lld Dj=%d M=%d invalid", (long long)N, Dj, M);
  return VCMI_OK;
}
int64_t first_bad_variance(const double *var, int Dj, int M) {
  for (int64_t e = 0; e < (int64_t)Dj * M; ++e)
    if (!(var[e] > 0.0)) return e;
  return -1;
}

int mfma_count_hook(DevBuf<unsigned long long> &count, int enable, int64_t *issued) {
  if (issued) {
    *issued = 0;
    if (count.p) {
      unsigned long long h = 0;
      VCMI_HIP(hipMemcpy(&h, count.p, sizeof(h), hipMemcpyDeviceToHost));
      *issued = (int64_t)h;
    }
  }
  if (enable) {
    if (!count.p) VCMI_TRY(count.alloc(1));
    VCMI_HIP(hipMemset(count.p, 0, sizeof(unsigned long long)));
  } else {
    count.release();
  }
  return VCMI_OK;
}

}  // namespace vcmi

using namespace vcmi;

extern "C" int64_t vcmi_estep_stats_len(int Dj, int M) { return estep_stats_len(Dj, M); }

extern "C" int vcmi_estep_diag_dev(const double *dX, int64_t N, int Dj, int M, const double *w, const double *mu,
                                   const double *var, double *dstats, void *stream) {
  return estep_device(dX, N, Dj, M, w, mu, var, dstats, as_stream(stream));
}

extern "C" int vcmi_estep_diag(const double *X, int64_t N, int Dj, int M, const double *w, const double *mu,
                               const double *var, double *S0, double *S1, double *S2, double *loglik) {
  if (!S0 || !S1 || !S2 || !loglik) return fail(VCMI_ERR_ARG, "vcmi_estep_diag: NULL output");
  VCMI_TRY(estep_check_dims(N, Dj, M));
  if (N > 0 && !X) return fail(VCMI_ERR_ARG, "vcmi_estep_diag: NULL frames");
  return estep_host(estep_device, X, N, Dj, M, w, mu, var, vcmi_estep_stats_len(Dj, M), (size_t)M * Dj, S0, S1, S2, loglik);
}

// Measurement hook (not part of include/vcmi.h; bench.py prices the diagonal E-step's matrix pipe with it): *issued (may be
// NULL) receives the v_mfma_f64_16x16x4 instructions the MFMA E-step kernels of THIS host thread have issued since the
// counter was last enabled; then enable != 0 (re)starts it at zero, enable == 0 switches it off.  Synchronises.
extern "C" int vcmi_debug_estep_mfma(int enable, int64_t *issued) { return vcmi::mfma_count_hook(vcmi::scratch().mfma_count, enable, issued); }

// Measurement hook (not part of include/vcmi.h): did the last diagonal E-step of this host thread take the hard-assignment
// path (estep_hard.hpp), and how many of its frames were soft (went through estep_mfma_kernel)?  *soft = -1: the one-kernel
// path.  Synchronises with the device.
extern "C" int vcmi_debug_estep_last_soft(int64_t *soft) {
  if (!soft) return fail(VCMI_ERR_ARG, "vcmi_debug_estep_last_soft: NULL argument");
  EstepScratch &sc = scratch();
  *soft = -1;
  if (sc.last_hard && sc.ctl.p) {
    int64_t h[kCtlLen];
    VCMI_HIP(hipDeviceSynchronize());
    VCMI_HIP(hipMemcpy(h, sc.ctl.p, sizeof(h), hipMemcpyDeviceToHost));
    if (h[kCtlHard]) *soft = h[kCtlNSoft];
  }
  return VCMI_OK;
}

extern "C" int vcmi_estep_set_path(int path) {
  if (path != VCMI_ESTEP_AUTO && path != VCMI_ESTEP_HARD && path != VCMI_ESTEP_SOFT)
    return fail(VCMI_ERR_ARG, "vcmi_estep_set_path: %d is not VCMI_ESTEP_AUTO / _HARD / _SOFT", path);
  estep_path_choice_ref() = path;
  return VCMI_OK;
}
extern "C" int vcmi_estep_get_path(int *path) {
  if (!path) return fail(VCMI_ERR_ARG, "vcmi_estep_get_path: NULL argument");
  *path = estep_path_choice_ref();
  return VCMI_OK;
}
