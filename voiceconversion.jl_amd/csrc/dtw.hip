// dtw.hip -- batched dynamic time warping + align post-processing on MI355X (gfx950).
//
// Replaces   fit!(d::DTW, template, sequence) + backward(d)    reference src/dtw.jl:93-145
//            lazy_init!(d, S, T)                               reference src/dtw.jl:44-51
//            transition / observation                          reference src/dtw.jl:23-35
//            align(src, tgt)                                   reference src/align.jl:8-35
//
// This file and the two that hold the kernels (dtw_fused.hip, dtw_twokernel.hip) are compiled with
// -ffp-contract=off: the parity contract for DTW is BIT-EXACT cost tables and back-pointers against the CPU oracle, whose arithmetic is  o = sum_d (v_d - tmpl_d)^2  accumulated
// sequentially in d with separately rounded multiply and add, and  cost = (C[j,t] + o) + transition.
// A GEMM-form distance or a fused multiply-add would change roundings and is therefore not used.
//
// Parallelisation.  Column t+1 of the cost table depends only on column t (src/dtw.jl:110,117), so the S rows
// of a column are independent: one workgroup owns a pair, thread r owns template frame r (its D values live in
// registers), the previous cost column is double-buffered in LDS and one s_barrier separates columns.
// Back-pointers are kept as small step codes (row - predecessor + fstep), 2 bits per cell packed 16 columns
// per LDS word when bstep+fstep <= 3, so the backward pass never touches HBM; the full Float64 / Int64 tables
// of the reference (d.costtable, d.backpointer) are streamed to HBM only when the caller asks for them.
//
// Here: the C entries, the host-pointer batch, the dispatcher dtw_run and the pad kernel that both paths launch.  The fused
// path (fstep = 0, bstep in {1,2}, D <= 48, path-only) is dtw_fused.hip, with its job list planned by dtw_plan.cpp; the
// observation + recurrence kernels and the generic kernel are dtw_twokernel.hip; dtw_device.hpp holds the device functions
// the kernels share, dtw_internal.hpp the scratch and the declarations that cross files.
#include "dtw_internal.hpp"
#include "devgroup.hpp"
#include "hostpipe.hpp"

#include <algorithm>

namespace vcmi {

// zero-pads the sequence and the template of every pair to DMAX doubles per frame (only launched when D != DMAX), so
// that the observation loop is branch-free: (0 - 0)^2 = +0.0 added to a non-negative sum leaves it bit-identical.
__global__ void __launch_bounds__(256)
dtw_pad_kernel(const double *__restrict__ feats, const DtwPair *__restrict__ pairs, int D, int DMAX, double *__restrict__ spad) {
  const DtwPair P = pairs[blockIdx.x];
  const int64_t ns = (int64_t)P.T * DMAX, nt = (int64_t)P.S * DMAX;
  for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < ns + nt; e += (int64_t)gridDim.y * 256) {
    const bool isseq = e < ns;
    const int64_t k = isseq ? e : e - ns;
    const int64_t f = k / DMAX;
    const int d = (int)(k % DMAX);
    const double v = (d < D) ? feats[(isseq ? P.seq_off : P.tmpl_off) + f * D + d] : 0.0;
    spad[(isseq ? P.spad_off : P.tpad_off) + k] = v;
  }
}
// the one launch site of the pad kernel (both paths call it, so the kernel lives in one code object)
void dtw_launch_pad(const double *feats, const DtwPair *dpairs, int n, int D, int dmax, double *spad, hipStream_t st) {
  hipLaunchKernelGGL(dtw_pad_kernel, dim3(n, 8), dim3(256), 0, st, feats, dpairs, D, dmax, spad);
}

static DtwScratch &scratch() {
  static thread_local DtwScratch s;
  return s;
}

// Validates a call, orders it behind the previous call's use of the scratch and hands it to the fused path or to the
// two-kernel / generic path.  `pairs` holds DEVICE pointers; the path taken sorts it and fills in its workspace offsets.
static int dtw_run(const double *feats, std::vector<DtwPair> &pairs, int D, int fstep, int bstep, DtwScratch &sc, hipStream_t st) {
  const int n = (int)pairs.size();
  if (n == 0) return VCMI_OK;
  VCMI_TRY(sc.init());
  VCMI_HIP(hipStreamWaitEvent(st, sc.last_use, 0));   // the workspaces may still be read by the previous call's kernels
  if (D < 1) return fail(VCMI_ERR_DIM, "DTW: feature dimension %d invalid", D);
  if (fstep < 0 || bstep < 0 || fstep + bstep > 255) return fail(VCMI_ERR_ARG, "DTW: fstep/bstep out of range");
  int Smax = 0, Tmax = 0;
  for (auto &p : pairs) {
    if (p.S < 1) return fail(VCMI_ERR_DIM, "DTW: template must have at least one frame");
    Smax = std::max(Smax, p.S);
    Tmax = std::max(Tmax, p.T);
  }
  if (Tmax == 0) return VCMI_OK;
  {
    bool tables = false;
    for (auto &p : pairs) tables = tables || p.cost || p.bp;
    if (fstep == 0 && (bstep == 1 || bstep == 2) && D <= kFusedMaxD && !tables && !debug_flag(kDbgDtwTwoKernels) &&
        dtw_fused_fits(Smax, Tmax))
      return dtw_run_fused(feats, pairs, D, bstep, sc, st, Smax, Tmax);
  }
  return dtw_run_twokernel(feats, pairs, D, fstep, bstep, sc, st, Smax, Tmax);
}

// Host-pointer batch on the current device: the feature matrices are gathered straight into the pinned staging slots
// (no intermediate host copy), run, and paths / tables / newtgt come back through the same ring.
static int dtw_host_batch_local(int64_t n, const double *const *tmpl, const int64_t *S, const double *const *seq,
                                const int64_t *T, int D, int fstep, int bstep, int64_t *const *path, double *cost,
                                int64_t *bp, double *const *newtgt) {
  VCMI_TRY(check_device());
  DtwScratch &sc = scratch();
  size_t nfeat = 0, npath = 0, ntgt = 0;
  for (int64_t p = 0; p < n; ++p) {
    nfeat += (size_t)D * (S[p] + T[p]);
    npath += (size_t)T[p];
    ntgt += (size_t)D * S[p];
  }
  VCMI_TRY(sc.feats.reserve(nfeat));
  VCMI_TRY(sc.paths.reserve(std::max<size_t>(npath, 1)));
  if (newtgt) VCMI_TRY(sc.newtgt.reserve(ntgt));
  const bool tables = (cost || bp);
  if (tables) {   // single-pair entry point only
    VCMI_TRY(sc.cost.reserve((size_t)S[0] * (T[0] + 1)));
    VCMI_TRY(sc.bp.reserve((size_t)S[0] * (T[0] + 1)));
  }
  std::vector<DtwPair> pairs(n);
  std::vector<HostPiece> up;
  up.reserve((size_t)2 * n);
  size_t fo = 0, po = 0, to = 0;
  for (int64_t p = 0; p < n; ++p) {
    DtwPair &q = pairs[p];
    up.push_back(HostPiece{const_cast<double *>(tmpl[p]), sizeof(double) * D * S[p]});
    q.tmpl_off = (int64_t)fo;
    fo += (size_t)D * S[p];
    if (T[p] > 0) up.push_back(HostPiece{const_cast<double *>(seq[p]), sizeof(double) * D * T[p]});
    q.seq_off = (int64_t)fo;
    fo += (size_t)D * T[p];
    q.path = sc.paths.p + po;
    po += (size_t)T[p];
    q.cost = tables ? sc.cost.p : nullptr;
    q.bp = tables ? sc.bp.p : nullptr;
    q.newtgt = newtgt ? sc.newtgt.p + to : nullptr;
    to += (size_t)D * S[p];
    q.codes = nullptr;
    q.obs_off = 0;
    q.spad_off = 0;
    q.tpad_off = 0;
    q.S = (int32_t)S[p];
    q.T = (int32_t)T[p];
  }
  VCMI_TRY(staged_upload_gather(sc.feats.p, up, nullptr));
  if (tables && T[0] == 0) {   // lazy_init! only: column 1 = 1:S
    for (int64_t i = 0; i < S[0]; ++i) {
      if (cost) cost[i] = (double)(i + 1);
      if (bp) bp[i] = i + 1;
    }
  }
  std::vector<DtwPair> order = pairs;   // dtw_run sorts its argument; keep `pairs` in caller order for the copy-back
  VCMI_TRY(dtw_run(sc.feats.p, order, D, fstep, bstep, sc, nullptr));
  if (path && npath > 0) {
    std::vector<HostPiece> down;
    std::vector<int64_t> dummy;
    bool all = true;
    for (int64_t p = 0; p < n; ++p) all = all && (path[p] != nullptr || T[p] == 0);
    if (all) {
      for (int64_t p = 0; p < n; ++p)
        if (T[p] > 0) down.push_back(HostPiece{path[p], sizeof(int64_t) * T[p]});
      VCMI_TRY(staged_download_scatter(down, sc.paths.p, nullptr));
    } else {   // some pairs want no path: take everything, hand out what was asked for
      dummy.resize(npath);
      VCMI_TRY(staged_download(dummy.data(), sc.paths.p, npath * 8, nullptr));
      po = 0;
      for (int64_t p = 0; p < n; ++p) {
        if (path[p] && T[p] > 0) memcpy(path[p], &dummy[po], sizeof(int64_t) * T[p]);
        po += (size_t)T[p];
      }
    }
  }
  if (newtgt) {
    // aligned targets: contiguous on the device in pair order; pairs without a sequence are all-zero (src/align.jl:19)
    std::vector<HostPiece> down;
    bool contiguous = true;
    for (int64_t p = 0; p < n; ++p) contiguous = contiguous && newtgt[p] && T[p] > 0;
    if (contiguous) {
      for (int64_t p = 0; p < n; ++p) down.push_back(HostPiece{newtgt[p], sizeof(double) * D * S[p]});
      VCMI_TRY(staged_download_scatter(down, sc.newtgt.p, nullptr));
    } else {
      VCMI_HIP(hipStreamSynchronize(nullptr));
      to = 0;
      for (int64_t p = 0; p < n; ++p) {
        if (newtgt[p]) {
          if (T[p] > 0) VCMI_HIP(hipMemcpy(newtgt[p], sc.newtgt.p + to, sizeof(double) * D * S[p], hipMemcpyDeviceToHost));
          else memset(newtgt[p], 0, sizeof(double) * D * S[p]);
        }
        to += (size_t)D * S[p];
      }
    }
  }
  if (tables && T[0] > 0) {
    if (cost) VCMI_TRY(staged_download(cost, sc.cost.p, sizeof(double) * S[0] * (T[0] + 1), nullptr));
    if (bp) VCMI_TRY(staged_download(bp, sc.bp.p, sizeof(int64_t) * S[0] * (T[0] + 1), nullptr));
  }
  VCMI_HIP(hipStreamSynchronize(nullptr));
  return VCMI_OK;
}

// pairs below which a batch stays on one device even when a device group is set
static constexpr int64_t kGroupMinPairs = 8;

// Pairs are independent: with a device group they are split by cost S*T (longest-processing-time) and every
// member aligns its share on its own device; no collective.
static int dtw_host_batch(int64_t n, const double *const *tmpl, const int64_t *S, const double *const *seq,
                          const int64_t *T, int D, int fstep, int bstep, int64_t *const *path, double *cost,
                          int64_t *bp, double *const *newtgt, bool allow_group = true) {
  if (n < 0) return fail(VCMI_ERR_ARG, "DTW: negative batch size");
  if (n == 0) return VCMI_OK;
  if (!tmpl || !S || !seq || !T) return fail(VCMI_ERR_ARG, "DTW: NULL argument");
  if (D < 1) return fail(VCMI_ERR_DIM, "DTW: feature dimension %d invalid", D);
  for (int64_t p = 0; p < n; ++p) {
    if (S[p] < 1 || T[p] < 0 || S[p] > INT32_MAX || T[p] > INT32_MAX) return fail(VCMI_ERR_DIM, "DTW: bad sequence length");
    if (!tmpl[p] || (T[p] > 0 && !seq[p])) return fail(VCMI_ERR_ARG, "DTW: NULL feature matrix");
  }
  const int m = group_size();
  if (!allow_group || m == 0 || n < kGroupMinPairs || cost || bp)
    return dtw_host_batch_local(n, tmpl, S, seq, T, D, fstep, bstep, path, cost, bp, newtgt);
  std::vector<int64_t> costs((size_t)n);
  for (int64_t p = 0; p < n; ++p) costs[(size_t)p] = S[p] * std::max<int64_t>(T[p], 1);
  const std::vector<int> part = shard_by_cost(costs, m);
  return group_run(m, [&](int i) -> int {
    std::vector<const double *> t2, s2;
    std::vector<int64_t> S2, T2;
    std::vector<int64_t *> p2;
    std::vector<double *> n2;
    for (int64_t p = 0; p < n; ++p) {
      if (part[(size_t)p] != i) continue;
      t2.push_back(tmpl[p]);
      s2.push_back(seq[p]);
      S2.push_back(S[p]);
      T2.push_back(T[p]);
      if (path) p2.push_back(path[p]);
      if (newtgt) n2.push_back(newtgt[p]);
    }
    if (t2.empty()) return VCMI_OK;
    return dtw_host_batch_local((int64_t)t2.size(), t2.data(), S2.data(), s2.data(), T2.data(), D, fstep, bstep,
                                path ? p2.data() : nullptr, nullptr, nullptr, newtgt ? n2.data() : nullptr);
  });
}

// align(src_p, tgt_p) for a batch, results LEFT ON THE DEVICE (dataset.hip builds the training matrix from them):
// *d_feats + src_off[p] is src_p (D,S_p), *d_newtgt + nt_off[p] the aligned target (D,S_p).  The buffers belong to the
// calling thread's DTW scratch and stay valid until its next DTW / align call.
int dtw_align_on_device(int64_t n, const double *const *src, const int64_t *S, const double *const *tgt, const int64_t *T,
                        int D, const double **d_feats, const double **d_newtgt, std::vector<int64_t> &src_off,
                        std::vector<int64_t> &nt_off) {
  std::vector<double *> nulls((size_t)std::max<int64_t>(n, 1), nullptr);
  // results stay in THIS thread's scratch on the current device: never spread over a device group
  VCMI_TRY(dtw_host_batch(n, src, S, tgt, T, D, /*fstep=*/0, /*bstep=*/2, nullptr, nullptr, nullptr, nulls.data(), false));
  DtwScratch &sc = scratch();
  *d_feats = sc.feats.p;
  *d_newtgt = sc.newtgt.p;
  src_off.resize((size_t)n);
  nt_off.resize((size_t)n);
  int64_t fo = 0, to = 0;
  for (int64_t p = 0; p < n; ++p) {
    src_off[p] = fo;
    nt_off[p] = to;
    fo += (int64_t)D * (S[p] + T[p]);
    to += (int64_t)D * S[p];
  }
  return VCMI_OK;
}

}  // namespace vcmi

using namespace vcmi;

extern "C" int vcmi_dtw_fit(const double *tmpl, int64_t S, const double *seq, int64_t T, int D, int fstep, int bstep,
                            int64_t *path, double *costtable, int64_t *backpointer) {
  int64_t *paths[1] = {path};
  const double *tp[1] = {tmpl}, *sp[1] = {seq};
  return dtw_host_batch(1, tp, &S, sp, &T, D, fstep, bstep, paths, costtable, backpointer, nullptr);
}

extern "C" int vcmi_dtw_fit_batch(int64_t n, const double *const *tmpl, const int64_t *S, const double *const *seq,
                                  const int64_t *T, int D, int fstep, int bstep, int64_t *const *path) {
  if (n > 0 && !path) return fail(VCMI_ERR_ARG, "vcmi_dtw_fit_batch: NULL path array");
  return dtw_host_batch(n, tmpl, S, seq, T, D, fstep, bstep, path, nullptr, nullptr, nullptr);
}

extern "C" int vcmi_dtw_fit_batch_dev(int64_t n, const double *feats, const int64_t *tmpl_off, const int64_t *S,
                                      const int64_t *seq_off, const int64_t *T, int D, int fstep, int bstep,
                                      int64_t *paths, const int64_t *path_off, void *stream) {
  if (n < 0) return fail(VCMI_ERR_ARG, "vcmi_dtw_fit_batch_dev: negative batch size");
  if (n == 0) return VCMI_OK;
  if (!feats || !tmpl_off || !S || !seq_off || !T || !paths || !path_off)
    return fail(VCMI_ERR_ARG, "vcmi_dtw_fit_batch_dev: NULL argument");
  std::vector<DtwPair> pairs(n);
  for (int64_t p = 0; p < n; ++p) {
    if (S[p] < 1 || T[p] < 0 || S[p] > INT32_MAX || T[p] > INT32_MAX) return fail(VCMI_ERR_DIM, "DTW: bad sequence length");
    DtwPair q{};
    q.tmpl_off = tmpl_off[p];
    q.seq_off = seq_off[p];
    q.path = paths + path_off[p];
    q.S = (int32_t)S[p];
    q.T = (int32_t)T[p];
    pairs[p] = q;
  }
  DtwScratch &sc = scratch();
  return dtw_run(feats, pairs, D, fstep, bstep, sc, as_stream(stream));
}

extern "C" int vcmi_align(const double *src, int64_t S, const double *tgt, int64_t T, int D, double *newtgt,
                          int64_t *path) {
  if (!newtgt) return fail(VCMI_ERR_ARG, "vcmi_align: NULL output");
  int64_t *paths[1] = {path};
  const double *tp[1] = {src}, *sp[1] = {tgt};
  double *nt[1] = {newtgt};
  return dtw_host_batch(1, tp, &S, sp, &T, D, /*fstep=*/0, /*bstep=*/2, paths, nullptr, nullptr, nt);   // src/align.jl:16
}

extern "C" int vcmi_align_batch(int64_t n, const double *const *src, const int64_t *S, const double *const *tgt,
                                const int64_t *T, int D, double *const *newtgt) {
  if (n > 0 && !newtgt) return fail(VCMI_ERR_ARG, "vcmi_align_batch: NULL output array");
  return dtw_host_batch(n, src, S, tgt, T, D, 0, 2, nullptr, nullptr, nullptr, newtgt);
}
