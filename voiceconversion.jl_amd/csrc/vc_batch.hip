// vc_batch.hip -- vc over a whole batch of utterances in one call (include/vcmi.h: vcmi_vc_frames_batch, vcmi_vc_traj_batch,
// vcmi_vc_trajgv_batch and the two *_batch_dev forms).
//
// The rule: result u of the batch is what vc(c_u, fm_u) gives on a fresh converter c_u with length(c_u) = length(c) -- chunks,
// deltas (bin/vc.jl:75-82, src/datasets.jl:6-13) and the post-filter's statistics (src/gv.jl:10-15) are per utterance.  The
// frames of all utterances lie back to back in one packed matrix; the chunks of all utterances are ONE TrajUtt list for one
// traj_run (vc_traj_device's loop with an outer utterance index), the frame-by-frame converter sees one (D+1, sum T) matrix.
// What is per utterance runs in three segmented kernels over host-made work lists (vc_batch_plan.cpp), so no thread searches
// the utterance boundaries:
//   vcb_pre_kernel    (utterance, 128-frame tile) items: every input element read once -> packed converter input (2D, sum T)
//                     and the power rows; static input gets its deltas with vc_traj_pre_kernel's arithmetic, edges per utterance
//   vcb_stat_*        (utterance, 2048-frame chunk) items + one finalisation per utterance: vs_partial_kernel / vs_final_kernel's
//                     summation order exactly (NG = 256 / D strided frame groups, the groups in order, the chunks in order, fma for
//                     the squares), so an utterance's mean and variance carry the bits of the single call
//   vcb_post_kernel   (utterance, tile) items: rows 2..D+1 of every result through fvpostf!'s scale (one [mean | var] pair per
//                     utterance) or copied
// All three are HBM-bound streaming passes: a tile is one contiguous range of memory and lane i takes element i of it.
#include "vc_batch_plan.hpp"
#include "traj_internal.hpp"
#include "hostpipe.hpp"
#include "postf.hpp"

#include <algorithm>

namespace vcmi {

// ---- kernel 1: fm_u (R+1, T_u) dense, read once -> x (2D, sum T) dense and row 1 of the results ---------------------------
// STATIC: R = D, x = [fm[2:end,:]; delta]; else R = 2D, x = fm[2:end,:]
template <bool STATIC>
__global__ void __launch_bounds__(256)
vcb_pre_kernel(const VcbUtt *__restrict__ utts, const VcbItem *__restrict__ tiles, const double *__restrict__ fm, int D,
               double *__restrict__ x, double *__restrict__ out) {
  const VcbItem it = tiles[blockIdx.x];
  const VcbUtt U = utts[it.utt];
  const int R = STATIC ? D : 2 * D, ld = R + 1;
  const int64_t t0 = it.first, T = U.T;
  const int nf = (int)((T - t0 < kVcbTileFrames) ? T - t0 : kVcbTileFrames);
  const double *src = fm + U.in_off;
  for (int e = threadIdx.x; e < nf * ld; e += 256) {
    const int tl = e / ld, r = e - tl * ld;
    const int64_t t = t0 + tl;
    const double v = src[t * ld + r];
    if (r == 0) {
      out[U.out_off + t * (D + 1)] = v;                              // power row kept, src/common.jl:60
      continue;
    }
    const int d = r - 1;
    double *xf = x + (U.frame0 + t) * 2 * D;
    xf[d] = v;
    // t = 2:T-1 of THIS utterance: -0.5 x_{t-1} + 0.5 x_{t+1}, src/datasets.jl:9-11; its first and last frame keep the copy
    if (STATIC) xf[D + d] = (t >= 1 && t + 1 < T) ? -0.5 * src[(t - 1) * ld + r] + 0.5 * src[(t + 1) * ld + r] : v;
  }
}

// ---- kernel 2: per-utterance mean and corrected variance, the order of vs_partial_kernel / vs_final_kernel (postf.hip) ------
// src: utterance u's converted rows at base + y_off(u) with leading dimension lds; stat: [n][mean (D) | var (D)]
template <int MODE>
__global__ void __launch_bounds__(256)
vcb_stat_partial_kernel(const VcbUtt *__restrict__ utts, const VcbItem *__restrict__ items, const double *__restrict__ base,
                        bool y_packed, int64_t lds, int D, const double *__restrict__ stat, double *__restrict__ part) {
  extern __shared__ double vred[];       // [NG][D]
  const VcbItem it = items[blockIdx.x];
  const VcbUtt U = utts[it.utt];
  const double *src = base + (y_packed ? U.frame0 * D : U.out_off + 1);
  const int tid = threadIdx.x, NG = 256 / D, d = tid % D, g = tid / D;
  const int64_t T = U.T, f0 = (int64_t)it.first * kVcbStatFrames, f1 = (f0 + kVcbStatFrames < T) ? f0 + kVcbStatFrames : T;
  double s = 0.0;
  if (g < NG) {
    const double m = MODE ? stat[(size_t)it.utt * 2 * D + d] : 0.0;
    for (int64_t t = f0 + g; t < f1; t += NG) {
      const double e = src[t * lds + d] - m;
      s = MODE ? fma(e, e, s) : s + e;
    }
    vred[g * D + d] = s;
  }
  __syncthreads();
  if (tid < D) {
    double a = 0.0;
    for (int k = 0; k < NG; ++k) a += vred[k * D + tid];
    part[(size_t)blockIdx.x * D + tid] = a;
  }
}

// one workgroup per utterance: stat[u][MODE][d] = (sum of its chunks' partial sums, in order) / (T_u - MODE)
__global__ void __launch_bounds__(256)
vcb_stat_final_kernel(const VcbUtt *__restrict__ utts, const int64_t *__restrict__ first, const double *__restrict__ part, int D,
                      int mode, double *__restrict__ stat) {
  const int u = blockIdx.x, d = threadIdx.x;
  if (d >= D) return;
  const int64_t c0 = first[u], c1 = first[u + 1];
  if (c0 == c1) return;                  // an empty utterance
  double a = 0.0;
  for (int64_t c = c0; c < c1; ++c) a += part[(size_t)c * D + d];
  stat[((size_t)u * 2 + mode) * D + d] = a / (double)(utts[u].T - mode);     // mode 1: Julia's var
}

// ---- kernel 3: rows 2..D+1 of every result, through fvpostf!'s scale (src/gv.jl:13, vs_scale_kernel's expression) or copied ---
// (src may be the result itself -- the frame-by-frame converter filters in place: every element is read and written by the
// same thread, hence no __restrict__ on the two)
template <bool FILTER>
__global__ void __launch_bounds__(256)
vcb_post_kernel(const VcbUtt *__restrict__ utts, const VcbItem *__restrict__ tiles, const double *base, bool y_packed, int64_t lds,
                int D, const double *__restrict__ stat, const double *__restrict__ sigma2, double *out) {
  const VcbItem it = tiles[blockIdx.x];
  const VcbUtt U = utts[it.utt];
  const int64_t t0 = it.first;
  const int nf = (int)((U.T - t0 < kVcbTileFrames) ? U.T - t0 : kVcbTileFrames);
  const double *src = base + (y_packed ? U.frame0 * D : U.out_off + 1);
  const double *mean = stat + (size_t)it.utt * 2 * D, *var = mean + D;
  double *dst = out + U.out_off + 1;
  for (int e = threadIdx.x; e < nf * D; e += 256) {
    const int tl = e / D, d = e - tl * D;
    const int64_t t = t0 + tl;
    const double xv = src[t * lds + d];
    dst[t * (D + 1) + d] = FILTER ? sqrt(sigma2[d] / var[d]) * (xv - mean[d]) + mean[d] : xv;
  }
}

// ---- the lists of a call on the device: per thread, grow-only, used under VcScratch::order like x and y ------------------------
struct VcbScratch {
  DevBuf<int64_t> lists;         // [utts | stat_first | tiles | stat_items] as 64-bit words (device-resident entries)
  DevBuf<double> part, stat;     // partial sums per statistics item; [n][mean | var] and sigma2 (D) behind them
};
static VcbScratch &vcb_scratch() {
  static thread_local VcbScratch s;
  return s;
}
struct VcbLists {
  const VcbUtt *utts;
  const int64_t *stat_first;
  const VcbItem *tiles, *stat_items;
};

// every list of the plan as one run of 64-bit words ...
static std::vector<int64_t> vcb_pack(const VcBatchPlan &p) {
  static_assert(sizeof(VcbUtt) == 32 && sizeof(VcbItem) == 8, "device images");
  const size_t n = p.utts.size(), w_utts = 4 * n, w_first = p.stat_first.size(), w_tiles = p.tiles.size(),
               w_items = p.stat_items.size();
  std::vector<int64_t> h(w_utts + w_first + w_tiles + w_items);
  if (n) memcpy(h.data(), p.utts.data(), sizeof(VcbUtt) * n);
  if (w_first) memcpy(h.data() + w_utts, p.stat_first.data(), 8 * w_first);
  if (w_tiles) memcpy(h.data() + w_utts + w_first, p.tiles.data(), 8 * w_tiles);
  if (w_items) memcpy(h.data() + w_utts + w_first + w_tiles, p.stat_items.data(), 8 * w_items);
  return h;
}
// ... and where each list is once the words lie at `words` on the device
static VcbLists vcb_lists_at(const VcBatchPlan &p, const int64_t *words) {
  const size_t w_utts = 4 * p.utts.size(), w_first = p.stat_first.size(), w_tiles = p.tiles.size();
  VcbLists d{};
  d.utts = reinterpret_cast<const VcbUtt *>(words);
  d.stat_first = words + w_utts;
  d.tiles = reinterpret_cast<const VcbItem *>(words + w_utts + w_first);
  d.stat_items = reinterpret_cast<const VcbItem *>(words + w_utts + w_first + w_tiles);
  return d;
}
// The device-resident entries upload them on their own, synchronously (model-sized data through the pinned ring, like the
// solver's descriptors); the host-pointer entries send them as one more piece of the gather that brings the utterances.
static int vcb_upload(const VcBatchPlan &p, VcbLists *d) {
  VcbScratch &sc = vcb_scratch();
  VCMI_TRY(upload_now(sc.lists, vcb_pack(p)));
  *d = vcb_lists_at(p, sc.lists.p);
  return VCMI_OK;
}

// statistics of every utterance (when sigma2) and the post kernel, on st.  base / y_packed / lds: where the converted rows are.
static int vcb_filter_and_post(const VcBatchPlan &p, const VcbLists &l, const double *base, bool y_packed, int64_t lds, int D,
                               const double *sigma2_host, double *dout, hipStream_t st) {
  const unsigned ntiles = (unsigned)p.tiles.size(), n = (unsigned)p.utts.size();
  if (!sigma2_host) {
    if (y_packed)
      hipLaunchKernelGGL(vcb_post_kernel<false>, dim3(ntiles), dim3(256), 0, st, l.utts, l.tiles, base, y_packed, lds, D, nullptr,
                         nullptr, dout);
    VCMI_HIP(hipGetLastError());
    return VCMI_OK;             // (in place without a filter: the rows are where they belong)
  }
  VcbScratch &sc = vcb_scratch();
  const unsigned nitems = (unsigned)p.stat_items.size();
  VCMI_TRY(sc.part.reserve((size_t)nitems * D));
  VCMI_TRY(sc.stat.reserve((size_t)n * 2 * D + D));
  double *sig = sc.stat.p + (size_t)n * 2 * D;
  // (D doubles from pageable memory: the runtime stages them before returning, the caller's vector is free at once)
  VCMI_HIP(hipMemcpyAsync(sig, sigma2_host, sizeof(double) * D, hipMemcpyHostToDevice, st));
  const size_t shm = (size_t)(256 / D) * D * sizeof(double);
  hipLaunchKernelGGL(vcb_stat_partial_kernel<0>, dim3(nitems), dim3(256), shm, st, l.utts, l.stat_items, base, y_packed, lds, D,
                     sc.stat.p, sc.part.p);
  hipLaunchKernelGGL(vcb_stat_final_kernel, dim3(n), dim3(256), 0, st, l.utts, l.stat_first, sc.part.p, D, 0, sc.stat.p);
  hipLaunchKernelGGL(vcb_stat_partial_kernel<1>, dim3(nitems), dim3(256), shm, st, l.utts, l.stat_items, base, y_packed, lds, D,
                     sc.stat.p, sc.part.p);
  hipLaunchKernelGGL(vcb_stat_final_kernel, dim3(n), dim3(256), 0, st, l.utts, l.stat_first, sc.part.p, D, 1, sc.stat.p);
  hipLaunchKernelGGL(vcb_post_kernel<true>, dim3(ntiles), dim3(256), 0, st, l.utts, l.tiles, base, y_packed, lds, D, sc.stat.p, sig,
                     dout);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// ---- trajectory converters ---------------------------------------------------------------------------------------------------
// Every check of a call, before anything is uploaded or launched; fills the plan and the GV parameters.
static int vcb_traj_check(const vcmi_traj *t, const vcmi_trajgv *gvh, int epochs, int64_t n, const int64_t *T, bool is_static,
                          const double *sigma2, const int64_t *in_off, const int64_t *out_off, VcBatchPlan *plan, TrajGV *gv,
                          const char *who) {
  VCMI_TRY(traj_two_windows_only(t, who, "vc over a batch of utterances"));     // (vcb_pre_kernel reads 2D feature rows)
  const int D = t->D;
  if (sigma2 && (D < 1 || D > 256)) return fail(VCMI_ERR_DIM, "%s: variance scaling needs 1 <= D <= 256", who);
  *plan = vc_batch_plan(n, T, true, t->length, (is_static ? D : t->D2) + 1, D + 1, sigma2 != nullptr, gvh != nullptr, in_off,
                        out_off);
  if (plan->status != VCMI_OK) return fail(plan->status, "%s: %s", who, plan->why);
  if (gvh) VCMI_TRY(trajgv_args(gvh, 0, nullptr, epochs, gv));     // (the one-frame chunks: the plan's verdict above)
  return VCMI_OK;
}

// The routine behind the four trajectory entries, vc_traj_device (traj_vc.cpp) with an outer utterance index: utterance u dense
// at dfm + in_off, its result dense at dout + out_off (the plan's offsets).  length(t) is left as it is.  dlists: the packed
// lists where the caller has already brought them to the device.
static int vc_traj_batch_device(vcmi_traj *t, const TrajGV *gv, const VcBatchPlan &plan, const double *dfm, bool is_static,
                                const double *sigma2, double *dout, hipStream_t st, const int64_t *dlists = nullptr) {
  const int64_t N = plan.nframes;
  if (N == 0) return VCMI_OK;
  const int D = t->D, D2 = t->D2;
  VCMI_TRY(check_device());
  VcScratch &sc = vc_scratch();
  TrajEmRelease em_release{t};
  VCMI_TRY(sc.x.reserve((size_t)D2 * N));
  VCMI_TRY(sc.y.reserve((size_t)D * N));
  VcbLists l{};
  if (dlists) l = vcb_lists_at(plan, dlists);       // (already on the device, in order before st's next work)
  else VCMI_TRY(vcb_upload(plan, &l));
  VCMI_TRY(sc.order.enter(st));
  const unsigned ntiles = (unsigned)plan.tiles.size();
  if (is_static) hipLaunchKernelGGL(vcb_pre_kernel<true>, dim3(ntiles), dim3(256), 0, st, l.utts, l.tiles, dfm, D, sc.x.p, dout);
  else hipLaunchKernelGGL(vcb_pre_kernel<false>, dim3(ntiles), dim3(256), 0, st, l.utts, l.tiles, dfm, D, sc.x.p, dout);
  VCMI_HIP(hipGetLastError());
  std::vector<TrajUtt> utts(plan.chunks.size());
  for (size_t k = 0; k < utts.size(); ++k) {
    const VcbChunk &c = plan.chunks[k];
    utts[k] = TrajUtt{sc.x.p + (size_t)c.frame0 * D2, sc.y.p + (size_t)c.frame0 * D, c.frame0, c.T, (int32_t)k};
  }
  VCMI_TRY(traj_run(t, utts, N, true, sc.x.p, st, gv));
  VCMI_TRY(vcb_filter_and_post(plan, l, sc.y.p, true, D, D, sigma2, dout, st));
  VCMI_TRY(sc.order.leave(st));
  return traj_check_status(t, st);
}

// host pointer arrays: gather (utterances and work lists) -> vc_traj_batch_device -> scatter
static int vc_traj_batch_host(vcmi_traj *t, vcmi_trajgv *gvh, int epochs, double alpha, int64_t n, const double *const *fm,
                              const int64_t *T, bool is_static, const double *sigma2, double *const *out, const char *who) {
  if (n < 0) return fail(VCMI_ERR_ARG, "%s: negative batch size", who);
  if (n == 0) return VCMI_OK;
  if (!fm || !T || !out) return fail(VCMI_ERR_ARG, "%s: NULL argument", who);
  VcBatchPlan plan;
  TrajGV gv{};
  gv.alpha = alpha;
  VCMI_TRY(vcb_traj_check(t, gvh, epochs, n, T, is_static, sigma2, nullptr, nullptr, &plan, &gv, who));
  for (int64_t u = 0; u < n; ++u)
    if (T[u] > 0 && (!fm[u] || !out[u])) return fail(VCMI_ERR_ARG, "%s: NULL matrix", who);
  const int64_t N = plan.nframes;
  if (N == 0) return VCMI_OK;
  VCMI_TRY(check_device());
  VcScratch &sc = vc_scratch();
  VcScratch::Release release{sc};   // on every way out
  const int D = t->D, rows = (is_static ? D : t->D2) + 1;
  const size_t nin = (size_t)rows * N, nout = (size_t)(D + 1) * N;
  std::vector<int64_t> lists = vcb_pack(plan);                       // staging matrix: [inputs | lists | results]
  VCMI_TRY(sc.stage.reserve(nin + lists.size() + nout));
  double *dlists = sc.stage.p + nin, *dout = dlists + lists.size();
  std::vector<HostPiece> up, down;
  for (int64_t u = 0; u < n; ++u) {
    if (T[u] == 0) continue;
    up.push_back(HostPiece{const_cast<double *>(fm[u]), sizeof(double) * rows * T[u]});
    down.push_back(HostPiece{out[u], sizeof(double) * (D + 1) * T[u]});
  }
  up.push_back(HostPiece{lists.data(), sizeof(int64_t) * lists.size()});
  VCMI_TRY(staged_upload_gather(sc.stage.p, up, nullptr));
  VCMI_TRY(vc_traj_batch_device(t, gvh ? &gv : nullptr, plan, sc.stage.p, is_static, sigma2, dout, nullptr,
                                reinterpret_cast<const int64_t *>(dlists)));
  return staged_download_scatter(down, dout, nullptr);
}

static int vc_traj_batch_dev(vcmi_traj *t, vcmi_trajgv *gvh, int epochs, double alpha, int64_t n, const double *dfm,
                             const int64_t *fm_off, const int64_t *T, bool is_static, const double *sigma2, double *dout,
                             const int64_t *out_off, hipStream_t st, const char *who) {
  if (n < 0) return fail(VCMI_ERR_ARG, "%s: negative batch size", who);
  if (n == 0) return VCMI_OK;
  if (!fm_off || !T || !out_off) return fail(VCMI_ERR_ARG, "%s: NULL argument", who);
  VcBatchPlan plan;
  TrajGV gv{};
  gv.alpha = alpha;
  VCMI_TRY(vcb_traj_check(t, gvh, epochs, n, T, is_static, sigma2, fm_off, out_off, &plan, &gv, who));
  if (plan.nframes > 0 && (!dfm || !dout)) return fail(VCMI_ERR_ARG, "%s: NULL buffer", who);
  return vc_traj_batch_device(t, gvh ? &gv : nullptr, plan, dfm, is_static, sigma2, dout, st);
}

}  // namespace vcmi

using namespace vcmi;

// vc(c::FrameByFrameConverter, fm_u) for every utterance: one conversion over the packed (D+1, sum T) matrix, then the
// per-utterance filter in place (vcmi_vc_frames_postf with an outer utterance index).  postf.hpp: vc_frames_batch.
int vcmi::vc_frames_batch(int D, const FrameConvertFn &convert, int64_t n, const double *const *fm, const int64_t *T,
                          const double *sigma2, double *const *out, const char *who) {
  if (n < 0) return fail(VCMI_ERR_ARG, "%s: negative batch size", who);
  if (n == 0) return VCMI_OK;
  if (!fm || !T || !out) return fail(VCMI_ERR_ARG, "%s: NULL argument", who);
  if (sigma2 && (D < 1 || D > 256)) return fail(VCMI_ERR_DIM, "%s: variance scaling needs 1 <= D <= 256", who);
  const VcBatchPlan plan = vc_batch_plan(n, T, false, 0, D + 1, D + 1, sigma2 != nullptr, false);
  if (plan.status != VCMI_OK) return fail(plan.status, "%s: %s", who, plan.why);
  for (int64_t u = 0; u < n; ++u)
    if (T[u] > 0 && (!fm[u] || !out[u])) return fail(VCMI_ERR_ARG, "%s: NULL matrix", who);
  const int64_t N = plan.nframes, ld = D + 1;
  if (N == 0) return VCMI_OK;
  VCMI_TRY(check_device());
  VcScratch &sc = vc_scratch();
  VcScratch::Release release{sc};
  std::vector<int64_t> lists;                                        // staging matrix: [inputs | lists | results]
  if (sigma2) lists = vcb_pack(plan);
  VCMI_TRY(sc.stage.reserve((size_t)2 * ld * N + lists.size()));
  double *din = sc.stage.p, *dlists = din + (size_t)ld * N, *dout = dlists + lists.size();
  std::vector<HostPiece> up, down;
  for (int64_t u = 0; u < n; ++u) {
    if (T[u] == 0) continue;
    up.push_back(HostPiece{const_cast<double *>(fm[u]), sizeof(double) * ld * T[u]});
    down.push_back(HostPiece{out[u], sizeof(double) * ld * T[u]});
  }
  if (!lists.empty()) up.push_back(HostPiece{lists.data(), sizeof(int64_t) * lists.size()});
  VCMI_TRY(staged_upload_gather(din, up, nullptr));
  // the copy keeps row 1 (src/common.jl:23); the kernel then overwrites rows 2..D+1, as in vcmi_vc_frames
  VCMI_HIP(hipMemcpyAsync(dout, din, sizeof(double) * ld * N, hipMemcpyDeviceToDevice, nullptr));
  VCMI_TRY(convert(din + 1, ld, N, dout + 1, nullptr));
  if (sigma2)
    VCMI_TRY(vcb_filter_and_post(plan, vcb_lists_at(plan, reinterpret_cast<const int64_t *>(dlists)), dout, false, ld, D, sigma2,
                                 dout, nullptr));
  return staged_download_scatter(down, dout, nullptr);
}

extern "C" int vcmi_vc_frames_batch(vcmi_gmmmap *g, int64_t n, const double *const *fm, const int64_t *T, const double *sigma2,
                                    double *const *out) {
  if (!g) return fail(VCMI_ERR_ARG, "vcmi_vc_frames_batch: NULL handle");
  return vc_frames_batch(g->D, [g](const double *dX, int64_t ld, int64_t N, double *dY, hipStream_t st) -> int {
                           return gmmmap_convert_device(g, dX, ld, N, dY, ld, st);
                         }, n, fm, T, sigma2, out, "vcmi_vc_frames_batch");
}

extern "C" int vcmi_vc_traj_batch(vcmi_traj *t, int64_t n, const double *const *fm, const int64_t *T, int is_static,
                                  const double *sigma2, double *const *out) {
  if (!t) return fail(VCMI_ERR_ARG, "vcmi_vc_traj_batch: NULL handle");
  return vc_traj_batch_host(t, nullptr, 0, 0.0, n, fm, T, is_static != 0, sigma2, out, "vcmi_vc_traj_batch");
}

extern "C" int vcmi_vc_trajgv_batch(vcmi_trajgv *h, int64_t n, const double *const *fm, const int64_t *T, int is_static, int epochs,
                                    double alpha, const double *sigma2, double *const *out) {
  if (!h) return fail(VCMI_ERR_ARG, "vcmi_vc_trajgv_batch: NULL handle");
  return vc_traj_batch_host(h->t, h, epochs, alpha, n, fm, T, is_static != 0, sigma2, out, "vcmi_vc_trajgv_batch");
}

extern "C" int vcmi_vc_traj_batch_dev(vcmi_traj *t, int64_t n, const double *dfm, const int64_t *fm_off, const int64_t *T,
                                      int is_static, const double *sigma2, double *dout, const int64_t *out_off, void *stream) {
  if (!t) return fail(VCMI_ERR_ARG, "vcmi_vc_traj_batch_dev: NULL handle");
  return vc_traj_batch_dev(t, nullptr, 0, 0.0, n, dfm, fm_off, T, is_static != 0, sigma2, dout, out_off, as_stream(stream),
                           "vcmi_vc_traj_batch_dev");
}

extern "C" int vcmi_vc_trajgv_batch_dev(vcmi_trajgv *h, int64_t n, const double *dfm, const int64_t *fm_off, const int64_t *T,
                                        int is_static, int epochs, double alpha, const double *sigma2, double *dout,
                                        const int64_t *out_off, void *stream) {
  if (!h) return fail(VCMI_ERR_ARG, "vcmi_vc_trajgv_batch_dev: NULL handle");
  return vc_traj_batch_dev(h->t, h, epochs, alpha, n, dfm, fm_off, T, is_static != 0, sigma2, dout, out_off, as_stream(stream),
                           "vcmi_vc_trajgv_batch_dev");
}
