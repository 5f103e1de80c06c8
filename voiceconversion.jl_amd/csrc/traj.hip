// traj.hip -- trajectory (MLPG) conversion with a GMM on static+delta features, MI355X (gfx950).
//
// Replaces   TrajectoryGMMMap ctor (Dy_m = inv(Syy_m - A_m Sxy_m))      reference src/trajectory_gmmmap.jl:11-31
//            constructW / compute_wt (never materialised: W is a stencil) reference src/trajectory_gmmmap.jl:39-61
//            fvconvert(tgmm, X)                                          reference src/trajectory_gmmmap.jl:65-110
//            vc(c::TrajectoryConverter, fm)                              reference src/common.jl:31-63
//            push_delta                                                  reference src/datasets.jl:6-13
//
// Math.  With mhat_t = argmax_m p(m | X_t), E_t = mu^y_m + A_m (X_t - mu^x_m), Q_t = Dy_mhat_t cut
// into DxD blocks [[Qss,Qsd],[Qds,Qdd]] and g_t = Q_t E_t = [gs; gd], the normal equations
// (W' Dy^-1 W) y = W' Dy^-1 E of :103-105 are block-pentadiagonal:
//   P[t,t]   = Qss(t) + Qdd(t-1)/4 + Qdd(t+1)/4        r[t] = gs(t) + gd(t-1)/2 - gd(t+1)/2
//   P[t,t-1] = Qds(t-1)/2 - Qsd(t)/2                   (terms with t-1 < 1 or t+1 > T dropped, as W drops them)
//   P[t,t-2] = -Qdd(t-1)/4
// One workgroup per utterance factorises P = L L' with a right-looking Cholesky on a sliding 3D x 3D window held
// in LDS (the right-hand side rides along as an extra row, so z = L^-1 r falls out of the same updates), streams
// the D-column panels of L to an HBM workspace, and back-substitutes L' y = z reading the panels in reverse.
// Here: the g_t kernels, traj_run, the batch routines and the convert entries; solvers: traj_solve.hip (diagonal precisions: traj_diag.hip), GV: traj_gv.hip, EM:
// traj_em.hip, vc: traj_vc.cpp, the constructor's arithmetic: traj_prepare.cpp (what crosses them: traj_internal.hpp).
#include "traj_internal.hpp"
#include "traj_prepare.hpp"
#include "devgroup.hpp"
#include "hostpipe.hpp"

#include <algorithm>
#include <memory>

namespace vcmi {

// ------------------------------------------------------------------------------------------------
// g_t = Q_mhat (A_mhat x_t + b_mhat): one workgroup per frame, thread r owns output row r
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(128)
traj_g_kernel(const double *__restrict__ X, int64_t nframes, int D2, const int64_t *__restrict__ mhat,
              const double *__restrict__ AT, const double *__restrict__ QT, const double *__restrict__ bvec,
              double *__restrict__ G) {
  extern __shared__ double sm[];   // x[D2], e[D2]
  double *xs = sm, *es = sm + D2;
  const int64_t fr = blockIdx.x;
  const int m = (int)mhat[fr] - 1;
  for (int r = threadIdx.x; r < D2; r += blockDim.x) xs[r] = X[fr * D2 + r];
  __syncthreads();
  const double *A = AT + (size_t)m * D2 * D2, *Q = QT + (size_t)m * D2 * D2;
  for (int r = threadIdx.x; r < D2; r += blockDim.x) {
    double e = bvec[(size_t)m * D2 + r];                       // E = mu^y + A (x - mu^x), src/trajectory_gmmmap.jl:88
    for (int k = 0; k < D2; ++k) e = fma(A[(size_t)k * D2 + r], xs[k], e);
    es[r] = e;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < D2; r += blockDim.x) {
    double s = 0.0;
    for (int k = 0; k < D2; ++k) s = fma(Q[(size_t)k * D2 + r], es[k], s);
    G[fr * D2 + r] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// g_t = Q_mhat (A_mhat x_t + b_mhat) on v_mfma_f64_16x16x4 (replaces one workgroup per frame streaming both 2D x 2D
// matrices from L2: 52 GB of L2 traffic per 512k frames).  One workgroup per utterance: frames grouped by mixture
// (counting sort, segments padded to 16), so a tile of 16 frames has ONE mixture; wave i owns row tile i of both
// products.  The two products chain without a layout change: register r of wave i's E accumulator (row 16i+4r+lane/16,
// frame lane%16) IS the B operand of k-step 4i+r of the second product for the same lane -- it only has to be shared
// with the other waves, through LDS.
// ------------------------------------------------------------------------------------------------
static constexpr int kGMaxKS = 24;   // k-steps of the widest supported feature vector (2D <= 96)
typedef double g_d4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(384)
traj_g_mfma_kernel(const TrajUtt *__restrict__ utts, int n, int D2, int M, int KS, const double *__restrict__ Afrag,
                   const double *__restrict__ Qfrag, const double *__restrict__ bvec, const int64_t *__restrict__ mhat_all,
                   int *__restrict__ perm_all, double *__restrict__ G_all, int split) {
  extern __shared__ double gsm2[];
  const int nthr = blockDim.x, NT = nthr >> 6;
  double *Xt = gsm2;                              // [4*KS][16] x of the tile's frames, k-major
  double *Ef = Xt + (size_t)4 * KS * 16;          // [4*NT][64] E accumulators in B-operand order (k-step major)
  int *cnt = reinterpret_cast<int *>(Ef + (size_t)4 * NT * 64);   // [M]
  int *start = cnt + M;                           // [M]
  __shared__ int tidx[16];
  __shared__ int ntiles_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lcol = lane & 15, lgrp = lane >> 4;
  // `split` (a power of two) workgroups share an utterance: a tile takes ~6 us of dependent loads and barriers and an
  // utterance has T / 16 and more of them -- with one workgroup per utterance and 256 utterances the kernel is a latency
  // chain on every CU.  Member `part` takes the tiles part, part + split, ... of the utterance's grouped order; every member
  // builds that order itself, so it has to be a function of the data: a STABLE counting sort (ranks by ballot / mbcnt per
  // wave, waves and chunks of frames in order), not one by atomics.  (Splitting by MIXTURE instead -- whole groups per
  // member, atomics allowed -- was measured first: a smooth trajectory stays in one or two mixtures, one member gets all the
  // tiles.)  The member index is the HIGH part of blockIdx: the members of an utterance sit on different XCDs.
  int *wcnt = start + M;                          // [NT][M] per-wave counts of the current chunk
  const int nutt = (int)(gridDim.x / (unsigned)split);
  const int part = (int)(blockIdx.x / (unsigned)nutt);
  for (int u = (int)(blockIdx.x % (unsigned)nutt); u < n; u += nutt) {
    const TrajUtt U = utts[u];
    const int T = U.T;
    if (T == 0) continue;
    const int64_t *mh = mhat_all + U.frame0;
    double *G = G_all + U.frame0 * D2;
    // regions indexed by the utterance's position in the batch (frame0 grows with it): disjoint whatever the launch order
    int *perm = perm_all + U.frame0 + (int64_t)16 * M * U.idx;
    // frames grouped by mixture, in frame order inside a group
    for (int m = tid; m < M; m += nthr) cnt[m] = 0;
    __syncthreads();
    for (int t = tid; t < T; t += nthr) atomicAdd(&cnt[(int)mh[t] - 1], 1);
    __syncthreads();
    if (tid == 0) {
      int pos = 0;
      for (int m = 0; m < M; ++m) {
        start[m] = pos;
        pos += (cnt[m] + 15) / 16 * 16;
        cnt[m] = 0;                                     // from here on: frames of mixture m placed so far
      }
      ntiles_s = pos / 16;
    }
    __syncthreads();
    const int ntiles = ntiles_s;
    for (int e = tid; e < ntiles * 16; e += nthr)
      if (((e >> 4) & (split - 1)) == part) perm[e] = -1;          // own tiles only
    for (int c0 = 0; c0 < T; c0 += nthr) {
      for (int e = tid; e < NT * M; e += nthr) wcnt[e] = 0;
      __syncthreads();
      const int t = c0 + tid;
      const int m = t < T ? (int)mh[t] - 1 : -1;
      int rank = 0;
      unsigned long long rem = __builtin_amdgcn_ballot_w64(m >= 0);
      while (rem) {                                     // one turn per distinct mixture among the wave's 64 frames
        const int lead = __builtin_ctzll(rem);
        const int k0 = __builtin_amdgcn_readlane(m, lead);
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(m == k0);
        if (m == k0) rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
        if (lane == lead) wcnt[wave * M + k0] = __builtin_popcountll(mask);
        rem &= ~mask;
      }
      __syncthreads();
      if (m >= 0) {
        int off = cnt[m] + rank;
        for (int w = 0; w < wave; ++w) off += wcnt[w * M + m];
        const int slot = start[m] + off;
        if (((slot >> 4) & (split - 1)) == part) perm[slot] = t;
      }
      __syncthreads();
      for (int m2 = tid; m2 < M; m2 += nthr) {
        int sum = 0;
        for (int w = 0; w < NT; ++w) sum += wcnt[w * M + m2];
        cnt[m2] += sum;
      }
      __syncthreads();
    }
    double afr[kGMaxKS], qfr[kGMaxKS];
    int mcur = -1;
    for (int tile = part; tile < ntiles; tile += split) {
      if (tid < 16) tidx[tid] = perm[tile * 16 + tid];
      __syncthreads();
      for (int e = tid; e < 4 * KS * 16; e += nthr) {
        const int k = e >> 4, t = tidx[e & 15];
        Xt[e] = (t >= 0 && k < D2) ? U.X[(size_t)t * D2 + k] : 0.0;
      }
      const int m = (int)mh[tidx[0]] - 1;               // slot 0 of a tile is never padding
      if (m != mcur) {
        mcur = m;
        const double *A = Afrag + (((size_t)m * NT + wave) * KS) * 64 + lane;
        const double *Q = Qfrag + (((size_t)m * NT + wave) * KS) * 64 + lane;
#pragma unroll
        for (int ks = 0; ks < kGMaxKS; ++ks) {
          afr[ks] = (ks < KS) ? A[(size_t)ks * 64] : 0.0;
          qfr[ks] = (ks < KS) ? Q[(size_t)ks * 64] : 0.0;
        }
      }
      g_d4 acc;                                         // E = A x + b, src/trajectory_gmmmap.jl:88
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wave + lgrp + 4 * r;
        acc[r] = (row < D2) ? bvec[(size_t)m * D2 + row] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < kGMaxKS; ++ks)
        if (ks < KS) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[ks], Xt[(4 * ks + lgrp) * 16 + lcol], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) Ef[(size_t)(4 * wave + r) * 64 + lane] = acc[r];
      __syncthreads();
      g_d4 gac = {0.0, 0.0, 0.0, 0.0};                  // g = Q E
#pragma unroll
      for (int ks = 0; ks < kGMaxKS; ++ks)
        if (ks < KS) gac = __builtin_amdgcn_mfma_f64_16x16x4f64(qfr[ks], Ef[(size_t)ks * 64 + lane], gac, 0, 0, 0);
      const int t = tidx[lcol];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wave + lgrp + 4 * r;
        if (row < D2 && t >= 0) G[(size_t)t * D2 + row] = gac[r];
      }
      __syncthreads();
    }
  }
}

int traj_run(vcmi_traj *t, std::vector<TrajUtt> &utts, int64_t nframes, bool contiguous, const double *dX0, hipStream_t st,
             const TrajGV *gv) {
  const int n = (int)utts.size();
  if (n == 0 || nframes == 0) return VCMI_OK;
  const int D2 = t->D2;
  VCMI_TRY(t->mhat.reserve((size_t)nframes));
  VCMI_TRY(t->gbuf.reserve((size_t)nframes * D2));
  // (1) mhat = predict(g.px, X), src/trajectory_gmmmap.jl:82
  // g_t on MFMA tiles (one workgroup per utterance); a cross-diagonal handle has made g_t in the arg-max pass
  const bool g_mfma = !t->b && t->NT <= 6 && !debug_flag(kDbgTrajGScalar);
  // diagonal conditional precisions: the same g_t kernels on the images of diag(q_m), then the tridiagonal solver
  const bool diag = t->precision == VCMI_TRAJ_PRECISION_DIAG;
  const double *QT = diag ? t->dg_QT.p : t->QT.p, *Qfrag = diag ? t->dg_Qfrag.p : t->Qfrag.p;
  auto arg_max = [&](const double *X, int64_t T, int64_t f0) -> int {     // ... and g_t where the scalar kernel runs
    if (t->b) return bdmap_traj_device(t->b, X, T, t->mhat.p + f0, t->gbuf.p + (size_t)f0 * D2, st);   // both, fused
    VCMI_TRY(gmmmap_predict_device(t->g, X, D2, T, t->mhat.p + f0, st, /*allow_screen=*/false));
    if (!g_mfma)
      hipLaunchKernelGGL(traj_g_kernel, dim3((unsigned)T), dim3(128), 2 * D2 * sizeof(double), st, X, T, D2, t->mhat.p + f0, t->AT.p,
                         QT, t->bvec.p, t->gbuf.p + (size_t)f0 * D2);
    return VCMI_OK;
  };
  if (contiguous) VCMI_TRY(arg_max(dX0, nframes, 0));
  for (auto &u : utts)
    if (!contiguous && u.T > 0) VCMI_TRY(arg_max(u.X, u.T, u.frame0));
  VCMI_HIP(hipGetLastError());
  // (2) banded solve
  int Tmax = 0;
  for (auto &u : utts) Tmax = std::max(Tmax, (int)u.T);
  VCMI_TRY(t->status.reserve(1));
  VCMI_TRY(t->uttbuf.reserve(sizeof(TrajUtt) * n));
  VCMI_HIP(hipMemsetAsync(t->status.p, 0, sizeof(int), st));
  // longest utterances first
  std::stable_sort(utts.begin(), utts.end(), [](const TrajUtt &a, const TrajUtt &b) { return a.T > b.T; });
  VCMI_TRY(upload_now(t->uttbuf.p, utts.data(), sizeof(TrajUtt) * n));
  const TrajUtt *du = reinterpret_cast<const TrajUtt *>(t->uttbuf.p);
  if (g_mfma) {
    const int cus = t->g->cus;      // (g_mfma: never a cross-diagonal handle, whose g is NULL)
    VCMI_TRY(t->gperm.reserve((size_t)nframes + (size_t)16 * t->M * n));
    const int nthr = 64 * t->NT;
    const size_t shg = ((size_t)4 * t->KS * 16 + (size_t)4 * t->NT * 64) * sizeof(double) + (2 + (size_t)t->NT) * (size_t)t->M * sizeof(int);
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(traj_g_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)shg));
    // workgroups per utterance: only while the batch leaves CUs idle (one utterance, or the twenty 100-frame chunks of one:
    // 328 -> ~70 us for 100 frames).  A batch that fills the chip gains nothing -- 256 x 2000 frames: 0.93 / 0.96 / 0.98 /
    // 1.05 ms with 1 / 2 / 4 / 8 members: there the kernel is bound by the A / Q fragments every change of mixture reloads
    // from L2 (102 KB each), not by the latency of a tile.
    int split = 1;
    while (split < 8 && (int64_t)n * 2 * split <= (int64_t)cus) split *= 2;
    hipLaunchKernelGGL(traj_g_mfma_kernel, dim3((unsigned)std::min<int64_t>((int64_t)n * split, (int64_t)4 * cus / split * split)),
                       dim3(nthr), shg, st, du, n, D2, t->M, t->KS, t->Afrag.p, Qfrag, t->bvec.p, t->mhat.p, t->gperm.p, t->gbuf.p, split);
    VCMI_HIP(hipGetLastError());
  }
  TrajSolvePlan plan;      // (its host work runs beside the g_t kernel)
  VCMI_TRY(traj_solve_plan(t, utts, nframes, Tmax, gv != nullptr, &plan));
  t->em_run_iters = 0;
  if (diag) {     // the band family, solver and ascent by t->windows
    VCMI_TRY(traj_band_solve_launch(t, plan, t->dg_q.p, t->mhat.p, st));
    // (EM: over a cross-diagonal handle with two windows only, vcmi_traj_set_em_bdiag refuses three)
    if (t->b && t->em_iters > 0) VCMI_TRY(traj_em_bdiag_run(t, utts, plan, st));
    // (GV: a handle of vcmi_trajgv_create_diag or _bdiag)
    if (gv && gv->epochs >= 0) VCMI_TRY(traj_band_gv_launch(t, plan, *gv, st));
    return VCMI_OK;
  }
  VCMI_TRY(traj_solve_launch(t, plan, plan.padded ? t->Qpad.p : t->Q.p, t->mhat.p, 0, n, st));
  if (t->em_iters > 0) VCMI_TRY(traj_em_run(t, utts, plan, contiguous, dX0, st));
  // (3) global-variance ascent on the solved trajectories, in place
  if (gv && gv->epochs >= 0) VCMI_TRY(traj_gv_launch(t, plan, *gv, st));
  return VCMI_OK;
}

int traj_two_windows_only(const vcmi_traj *t, const char *who, const char *what) {
  if (t->windows != 3) return VCMI_OK;
  return fail(VCMI_ERR_ARG, "%s: the converter has three windows (static + delta + delta-delta, vcmi_traj_create_bdiag_windows): %s "
                            "is provided for two windows only", who, what);
}

int traj_check_status(vcmi_traj *t, hipStream_t st) {
#ifdef TRAJ_BLK_PROF
  traj_solve_prof_dump(st);
  traj_gv_prof_dump(st);
#endif
  int h = 0;
  VCMI_HIP(hipMemcpyAsync(&h, t->status.p, sizeof(int), hipMemcpyDeviceToHost, st));
  VCMI_HIP(hipStreamSynchronize(st));
  // the EM objective of the call: L at each E-step, summed over the utterances in the caller's order
  t->em_hist.assign((size_t)t->em_run_iters, 0.0);
  if (t->em_run_iters > 0) {
    std::vector<double> L((size_t)t->em_run_iters * t->em_run_n);
    VCMI_HIP(hipMemcpy(L.data(), t->em_L.p, L.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int it = 0; it < t->em_run_iters; ++it)
      for (int u = 0; u < t->em_run_n; ++u) t->em_hist[(size_t)it] += L[(size_t)it * t->em_run_n + u];
    traj_em_release(t);
  }
  if (h) return fail(VCMI_ERR_NOT_PD, "trajectory normal matrix W'D^-1W is not positive definite");
  return VCMI_OK;
}

// host-pointer batch on the current device: the utterances are gathered straight into the pinned staging slots, run,
// and scattered back the same way
static int traj_host_batch_local(vcmi_traj *t, int64_t n, const double *const *X, const int64_t *T, double *const *Y,
                                 const TrajGV *gv) {
  int64_t nframes = 0;
  for (int64_t u = 0; u < n; ++u) nframes += T[u];
  t->em_hist.assign((size_t)t->em_iters, 0.0);
  if (nframes == 0) return VCMI_OK;
  TrajEmRelease em_release{t};
  const int D = t->D, D2 = t->D2;
  VCMI_TRY(t->xbuf.reserve((size_t)nframes * D2));
  VCMI_TRY(t->ybuf.reserve((size_t)nframes * D));
  std::vector<TrajUtt> utts(n);
  std::vector<HostPiece> up, down;
  int64_t f0 = 0;
  for (int64_t u = 0; u < n; ++u) {
    if (T[u] > 0) {
      up.push_back(HostPiece{const_cast<double *>(X[u]), sizeof(double) * D2 * T[u]});
      down.push_back(HostPiece{Y[u], sizeof(double) * D * T[u]});
    }
    utts[u] = TrajUtt{t->xbuf.p + (size_t)f0 * D2, t->ybuf.p + (size_t)f0 * D, f0, (int32_t)T[u], (int32_t)u};
    f0 += T[u];
  }
  VCMI_TRY(staged_upload_gather(t->xbuf.p, up, nullptr));
  VCMI_TRY(traj_run(t, utts, nframes, true, t->xbuf.p, nullptr, gv));
  VCMI_TRY(traj_check_status(t, nullptr));
  return staged_download_scatter(down, t->ybuf.p, nullptr);
}

// the replica list of a handle (vcmi_traj, vcmi_trajgv) follows the device group: emptied and resized when the group changed
template <class H>
static void reset_stale_replicas(H *h) {
  const uint64_t ep = group_epoch();
  if (h->replicas_epoch == ep && (int)h->replicas.size() == group_size()) return;
  for (H *r : h->replicas) delete r;
  h->replicas.assign((size_t)group_size(), nullptr);
  h->replicas_epoch = ep;
}

static void traj_sync_replicas(vcmi_traj *t) {
  if (!t->b) gmmmap_sync_replicas(t->g);
  reset_stale_replicas(t);
}

// member i's trajectory converter: t itself when member i got t's own GMMMap, else a replica over the member's GMMMap
static int traj_member(vcmi_traj *t, int member, vcmi_traj **out) {
  if (t->b) {     // (traj_host_batch keeps such a handle on its own device)
    *out = t;
    return VCMI_OK;
  }
  vcmi_gmmmap *g = nullptr;
  VCMI_TRY(gmmmap_member(t->g, member, &g));
  if (g == t->g) {
    *out = t;
    return VCMI_OK;
  }
  vcmi_traj *&r = t->replicas[(size_t)member];
  if (!r) VCMI_TRY(vcmi_traj_create(g, t->length, &r));
  r->em_iters = t->em_iters;      // the handle's settings, whenever they were made
  if (t->precision == VCMI_TRAJ_PRECISION_DIAG) VCMI_TRY(traj_diag_ensure(r));     // (on the member's device: its worker thread)
  r->precision = t->precision;
  *out = r;
  return VCMI_OK;
}

// utterances below which a batch stays on one device even when a device group is set
static constexpr int64_t kGroupMinUtts = 8;

// Utterances (and the chunks of vc) are independent: with a device group they are split by length
// (longest-processing-time) and every member converts its share on its own device; no collective.
int traj_host_batch(vcmi_traj *t, int64_t n, const double *const *X, const int64_t *T, double *const *Y, const TrajGV *gv,
                    vcmi_trajgv *gvh) {
  if (!t) return fail(VCMI_ERR_ARG, "trajectory: NULL handle");
  if (n < 0) return fail(VCMI_ERR_ARG, "trajectory: negative batch size");
  if (n == 0) return VCMI_OK;
  if (!X || !T || !Y) return fail(VCMI_ERR_ARG, "trajectory: NULL argument");
  for (int64_t u = 0; u < n; ++u) {
    if (T[u] < 0 || T[u] > INT32_MAX) return fail(VCMI_ERR_DIM, "trajectory: bad utterance length");
    if (T[u] > 0 && (!X[u] || !Y[u])) return fail(VCMI_ERR_ARG, "trajectory: NULL matrix");
  }
  const int m = group_size();
  // a cross-diagonal handle follows vcmi_bdmap's rule: it converts on the device it was created on, groups do not shard it
  if (m == 0 || n < kGroupMinUtts || t->b) return traj_host_batch_local(t, n, X, T, Y, gv);
  traj_sync_replicas(t);
  if (gvh) reset_stale_replicas(gvh);
  std::vector<int64_t> costs((size_t)n);
  for (int64_t u = 0; u < n; ++u) costs[(size_t)u] = T[u];
  const std::vector<int> part = shard_by_cost(costs, m);
  std::vector<std::vector<double>> hist((size_t)m);     // every member's EM objective
  const int rc = group_run(m, [&](int i) -> int {
    std::vector<const double *> x2;
    std::vector<double *> y2;
    std::vector<int64_t> T2;
    for (int64_t u = 0; u < n; ++u) {
      if (part[(size_t)u] != i) continue;
      x2.push_back(X[u]);
      y2.push_back(Y[u]);
      T2.push_back(T[u]);
    }
    if (x2.empty()) return VCMI_OK;
    vcmi_traj *r = nullptr;
    VCMI_TRY(traj_member(t, i, &r));
    TrajGV gv2;
    if (gv) {
      gv2 = *gv;
      if (r != t) {   // the GV statistics on this member's device
        vcmi_trajgv *&gr = gvh->replicas[(size_t)i];
        if (!gr) {
          gr = new (std::nothrow) vcmi_trajgv();
          if (!gr) return fail(VCMI_ERR_OOM, "out of host memory");
          gr->t = r;
          gr->diag = gvh->diag;
          VCMI_TRY(gr->muv.alloc(gvh->h_muv.size()));
          VCMI_TRY(gr->pv.alloc(gvh->h_pv.size()));
          VCMI_TRY(upload_now(gr->muv.p, gvh->h_muv.data(), gvh->h_muv.size() * 8));
          VCMI_TRY(upload_now(gr->pv.p, gvh->h_pv.data(), gvh->h_pv.size() * 8));
        }
        gv2.muv = gr->muv.p;
        gv2.pv = gr->pv.p;
      }
    }
    const int rcl = traj_host_batch_local(r, (int64_t)x2.size(), x2.data(), T2.data(), y2.data(), gv ? &gv2 : nullptr);
    hist[(size_t)i] = r->em_hist;
    return rcl;
  });
  t->em_hist.assign((size_t)t->em_iters, 0.0);
  for (auto &hm : hist)
    for (size_t k = 0; k < hm.size() && k < t->em_hist.size(); ++k) t->em_hist[k] += hm[k];
  return rc;
}

}  // namespace vcmi

using namespace vcmi;

extern "C" int vcmi_traj_create(vcmi_gmmmap *g, int64_t T, vcmi_traj **out) {
  if (!g || !out) return fail(VCMI_ERR_ARG, "vcmi_traj_create: NULL argument");
  *out = nullptr;
  if (g->D & 1) return fail(VCMI_ERR_DIM, "TrajectoryGMMMap: dim(g) = %d must be even (static + delta)", g->D);
  if (T < 0) return fail(VCMI_ERR_ARG, "TrajectoryGMMMap: negative length");
  TrajModel tm;     // the host arithmetic: traj_prepare.cpp
  VCMI_TRY(traj_prepare_model(g->h_A, g->h_Sxy, g->h_Syy, g->h_mux, g->h_muy, g->D, g->M, tm));
  std::unique_ptr<vcmi_traj> t(new (std::nothrow) vcmi_traj());
  if (!t) return fail(VCMI_ERR_OOM, "out of host memory");
  t->g = g;
  t->D2 = g->D;
  t->D = g->D / 2;
  t->M = g->M;
  t->length = T;
  t->big = traj_solve_is_big(t->D);
  t->NT = tm.NT;
  t->KS = tm.KS;
  t->Dpad = tm.Dpad;
  t->em_pd = tm.em_pd;
  const char *up = "TrajectoryGMMMap: upload failed: %s";
  const struct {
    DevBuf<double> &dev;
    const std::vector<double> &host;
    const char *msg;       // of a failed upload
  } images[] = {{t->Qpad, tm.Qpad, "vcmi_traj_create: upload of the padded Q failed"}, {t->Q, tm.Q, up}, {t->QT, tm.QT, up},
                {t->AT, tm.AT, up}, {t->bvec, tm.b, up}, {t->Qfrag, tm.Qfrag, up}, {t->Afrag, tm.Afrag, up}, {t->cm, tm.cm, up}};
  for (auto &im : images) {
    if (im.host.empty()) continue;     // (Qpad of a dimension with its own instantiation)
    VCMI_TRY(im.dev.alloc(im.host.size()));
    const hipError_t e = upload_now_hip(im.dev.p, im.host.data(), im.host.size() * 8);
    if (e != hipSuccess) return fail(VCMI_ERR_HIP, im.msg, hipGetErrorString(e));
  }
  *out = t.release();
  return VCMI_OK;
}

// TrajectoryGMMMap straight from a cross-diagonal model: the conditional covariance of every mixture is
// diagonal exactly, so the converter IS a diagonal-precision one -- q from the pairs (gmmmap_bdiag_prepare.cpp), nothing dense.
static int traj_create_bdiag(vcmi_bdmap *b, int64_t T, int windows, vcmi_traj **out, const char *who) {
  if (!b || !out) return fail(VCMI_ERR_ARG, "%s: NULL argument", who);
  *out = nullptr;
  if (windows != 2 && windows != 3) return fail(VCMI_ERR_ARG, "%s: %d windows: 2 (static + delta) or 3 (static + delta + delta-delta)", who, windows);
  if (windows == 2 && (b->D & 1)) return fail(VCMI_ERR_DIM, "TrajectoryGMMMap: dim(g) = %d must be even (static + delta)", b->D);
  if (windows == 3 && b->D % 3 != 0)
    return fail(VCMI_ERR_DIM, "TrajectoryGMMMap: dim(g) = %d must be a multiple of 3 (static + delta + delta-delta)", b->D);
  if (T < 0) return fail(VCMI_ERR_ARG, "TrajectoryGMMMap: negative length");
  if (b->q_bad >= 0)
    return fail(VCMI_ERR_NOT_PD, "%s: the conditional variance of pair (%d,%d) is not positive and finite", who,
                (int)(b->q_bad % b->D) + 1, (int)(b->q_bad / b->D) + 1);
  int dev = 0;
  VCMI_HIP(hipGetDevice(&dev));
  if (dev != b->device)
    return fail(VCMI_ERR_ARG, "%s: the handle was created on device %d, the call runs on device %d", who, b->device, dev);
  std::unique_ptr<vcmi_traj> t(new (std::nothrow) vcmi_traj());
  if (!t) return fail(VCMI_ERR_OOM, "out of host memory");
  t->b = b;
  t->D2 = b->D;
  t->windows = windows;
  t->D = b->D / windows;
  t->M = b->M;
  t->length = T;
  t->precision = VCMI_TRAJ_PRECISION_DIAG;
  VCMI_TRY(upload_now(t->dg_q, b->h_q));       // [M][dim(b)]: (dim(b),M) dimension fastest is that layout
  t->diag_ready = true;
  *out = t.release();
  return VCMI_OK;
}

extern "C" int vcmi_traj_create_bdiag(vcmi_bdmap *b, int64_t T, vcmi_traj **out) {
  return traj_create_bdiag(b, T, 2, out, "vcmi_traj_create_bdiag");
}

// ... over static + delta (windows = 2: vcmi_traj_create_bdiag exactly) or static + delta + delta-delta features (windows = 3,
// dim(b) = 3D, the pentadiagonal solver of traj_penta.hip)
extern "C" int vcmi_traj_create_bdiag_windows(vcmi_bdmap *b, int64_t T, int windows, vcmi_traj **out) {
  if (windows == 2) return vcmi_traj_create_bdiag(b, T, out);
  return traj_create_bdiag(b, T, windows, out, "vcmi_traj_create_bdiag_windows");
}
extern "C" int vcmi_traj_get_windows(const vcmi_traj *t) { return t ? t->windows : -1; }

extern "C" int vcmi_traj_destroy(vcmi_traj *t) {
  delete t;
  return VCMI_OK;
}
extern "C" int64_t vcmi_traj_length(const vcmi_traj *t) { return t ? t->length : -1; }

extern "C" int vcmi_traj_convert(vcmi_traj *t, const double *X, int64_t T, double *Y) {
  const double *xs[1] = {X};
  double *ys[1] = {Y};
  VCMI_TRY(traj_host_batch(t, 1, xs, &T, ys));
  // The reference rebuilds W when the sequence length differs from length(tgmm) (src/trajectory_gmmmap.jl:70-72), so
  // afterwards length(tgmm) == T -- and with it the chunk length of the next vc call (src/common.jl:41).  Reproduced.
  t->length = T;
  return VCMI_OK;
}

extern "C" int vcmi_traj_convert_batch(vcmi_traj *t, int64_t n, const double *const *X, const int64_t *T, double *const *Y) {
  return traj_host_batch(t, n, X, T, Y);
}

// the body of the two device-resident batch entries: utterance u has X at dX + x_off[u] and Y at dY + y_off[u]
static int traj_batch_device(vcmi_traj *t, const TrajGV *gv /* may be NULL */, int64_t n, const double *dX, const int64_t *x_off,
                             const int64_t *T, double *dY, const int64_t *y_off, hipStream_t st, const char *who) {
  if (n == 0) return VCMI_OK;
  if (!dX || !x_off || !T || !dY || !y_off) return fail(VCMI_ERR_ARG, "%s: NULL argument", who);
  std::vector<TrajUtt> utts(n);
  int64_t f0 = 0;
  bool contiguous = true;
  for (int64_t u = 0; u < n; ++u) {
    if (T[u] < 0 || T[u] > INT32_MAX) return fail(VCMI_ERR_DIM, "trajectory: bad utterance length");
    if (x_off[u] != x_off[0] + f0 * t->D2) contiguous = false;
    utts[u] = TrajUtt{dX + x_off[u], dY + y_off[u], f0, (int32_t)T[u], (int32_t)u};
    f0 += T[u];
  }
  t->em_hist.assign((size_t)t->em_iters, 0.0);
  if (f0 == 0) return VCMI_OK;   // only empty utterances: nothing was launched, there is no status to read
  TrajEmRelease em_release{t};
  VCMI_TRY(traj_run(t, utts, f0, contiguous, dX + x_off[0], st, gv));
  return traj_check_status(t, st);
}

extern "C" int vcmi_traj_convert_batch_dev(vcmi_traj *t, int64_t n, const double *dX, const int64_t *x_off, const int64_t *T,
                                           double *dY, const int64_t *y_off, void *stream) {
  if (!t) return fail(VCMI_ERR_ARG, "vcmi_traj_convert_batch_dev: NULL handle");
  if (n < 0) return fail(VCMI_ERR_ARG, "vcmi_traj_convert_batch_dev: negative batch size");
  return traj_batch_device(t, nullptr, n, dX, x_off, T, dY, y_off, as_stream(stream), "vcmi_traj_convert_batch_dev");
}

extern "C" int vcmi_trajgv_convert_batch(vcmi_trajgv *h, int64_t n, const double *const *X, const int64_t *T, int epochs,
                                         double alpha, double *const *Y) {
  TrajGV gv{};
  gv.alpha = alpha;
  VCMI_TRY(trajgv_args(h, n, T, epochs, &gv));
  return traj_host_batch(h->t, n, X, T, Y, &gv, h);
}

extern "C" int vcmi_trajgv_convert(vcmi_trajgv *h, const double *X, int64_t T, int epochs, double alpha, double *Y) {
  const double *xs[1] = {X};
  double *ys[1] = {Y};
  VCMI_TRY(vcmi_trajgv_convert_batch(h, 1, xs, &T, epochs, alpha, ys));
  h->t->length = T;   // fvconvert(tgv.tgmm, X) rebuilt W for this T, src/trajectory_gmmmap.jl:70-72,146
  return VCMI_OK;
}

extern "C" int vcmi_trajgv_convert_batch_dev(vcmi_trajgv *h, int64_t n, const double *dX, const int64_t *x_off, const int64_t *T,
                                             int epochs, double alpha, double *dY, const int64_t *y_off, void *stream) {
  TrajGV gv{};
  gv.alpha = alpha;
  VCMI_TRY(trajgv_args(h, n, T, epochs, &gv));
  if (n < 0) return fail(VCMI_ERR_ARG, "vcmi_trajgv_convert_batch_dev: negative batch size");
  return traj_batch_device(h->t, &gv, n, dX, x_off, T, dY, y_off, as_stream(stream), "vcmi_trajgv_convert_batch_dev");
}
