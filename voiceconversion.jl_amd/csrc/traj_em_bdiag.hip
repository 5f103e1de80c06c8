// traj_em_bdiag.hip -- EM re-estimation of the trajectory over ALL mixtures (Toda, Black, Tokuda 2007, eqs. 30-36) for a converter
// made straight from a CROSS-DIAGONAL model (vcmi_traj_create_bdiag): the fused E-step + M-step sums, the loop
// (traj_internal.hpp: traj_em_bdiag_run) and the vcmi_traj_*_bdiag entries (include/vcmi.h).  DESIGN 3.4-BDIAG-EM.
//
// Statement (restated in numpy in tests/traj_em_bdiag_restatement.py).  Per mixture m and feature k = 0 .. 2D-1, source side x and
// target side y after the swap:  l_tm the centred source log-density (BdmapTable::cst; -inf for w_m <= 0),  a = c / vx,
// q = 1 / (vy - a c),  E_kmt = muy_km + a_km (x_kt - mux_km),  Y_t(y) = (W y)_t = [y_t ; (y_{t+1} - y_{t-1}) / 2] with W's boundary
// rule (a missing neighbour is dropped),  c_m = 1/2 sum_k log q_km.
//   E-step   l'_mt = (l_tm - lse_m l_tm) + c_m - 1/2 sum_k q_km (Y_kt - E_kmt)^2 - D log 2 pi
//            lse_t = logsumexp_m l'_mt,  gamma_mt = exp(l'_mt - lse_t),  L(y) = sum_t lse_t = log P(W y | X)
//   M-step   qbar_kt = sum_m gamma_mt q_km,  gbar_kt = sum_m gamma_mt q_km E_kmt;  the tridiagonal systems of traj_diag.hip with
//            (qbar_t, gbar_t) in place of (q_mhat, g_t)
// y^0 is the arg-max solution; em_iters = n runs n E/M pairs.  This is traj_em.hip's statement with Q_m = diag(q_m).
//
// One kernel, one launch per iteration, in the shape of bdmap_kernel (gmmmap_bdiag.hip): a workgroup of eight waves takes FB
// consecutive frames of ONE utterance (a tile job of traj_em_bdiag_plan.hpp), lane = frame, parameters wave-uniform:
//   stage     x of the tile and Y = W y (the stencil over y, with the frame before and after the tile inside the utterance)
//             into LDS, xs[k][frame] and ys[k][frame]
//   phase 1a  wave w takes the mixtures 4 w .. 4 w + 3, then + 32, ...: l_tm, the sum over k ascending -> L[m][frame]
//   phase 2a  thread (part, frame): lse_m l of the frame, the NP partial results combined through LDS in a fixed order
//   phase 1b  the same mixtures: the target term over k ascending from the [mu_x, a, mu_y, q] rows; L <- (l - lse_m l) + (c_m -
//             D log 2 pi - 1/2 sum)
//   phase 2b  lse_t, then gamma in place (exp(-inf) = 0 exactly for w_m <= 0); lse_t goes to HBM; the L-only mode ends here
//   phase 3   wave w takes the features 2 w, 2 w + 1, then + 16, ...: qbar and gbar over all mixtures ascending; they take the
//             place of Y and x in LDS (each element read and written by the same lane)
//   store     one (FB, 2D) tile each to the qbar table and to gbar
// Nothing per (frame, mixture) goes to HBM, there are no atomics, and no index depends on the data: a frame's bits are a
// function of the model, the utterance and the frame, and a NaN frame gives NaN results and nothing else.
#include "traj_internal.hpp"
#include "traj_em_bdiag_plan.hpp"
#include "gmmmap_bdiag_prepare.hpp"
#include "hostpipe.hpp"

#include <cmath>

namespace vcmi {

// Maximum, sum and (IN_PLACE) quotient over the mixtures of a frame: thread (part, fr) takes the mixtures part, part + NP, ...;
// the partial results are combined in the order 0 .. NP-1 by every thread of the frame, so all of them hold the same bits.
// Returns logsumexp_m L[m][fr]; IN_PLACE: L <- exp(L - max) / sum.  Ends with L read for the last time BEFORE its last barrier
// unless IN_PLACE.
template <int FB, bool IN_PLACE>
__device__ __forceinline__ double em_bd_lse(double *L, double *red, int M, int fr, int part) {
  constexpr int NP = kEmBdThreads / FB;
  double u = -INFINITY;
  for (int m = part; m < M; m += NP) u = fmax(u, L[m * FB + fr]);
  red[part * FB + fr] = u;
  __syncthreads();
  u = red[fr];
  for (int k = 1; k < NP; ++k) u = fmax(u, red[k * FB + fr]);
  __syncthreads();
  double s = 0.0;
  for (int m = part; m < M; m += NP) {
    const double e = exp(L[m * FB + fr] - u);
    if (IN_PLACE) L[m * FB + fr] = e;
    s += e;
  }
  red[part * FB + fr] = s;
  __syncthreads();
  s = red[fr];
  for (int k = 1; k < NP; ++k) s += red[k * FB + fr];
  if (IN_PLACE)
    for (int m = part; m < M; m += NP) L[m * FB + fr] = L[m * FB + fr] / s;
  return u + log(s);
}

// LONLY: stop after phase 2b (vcmi_traj_cond_loglik_bdiag).  D2 = 2D features, DP = D2 rounded up to a multiple of four (the
// padding rows of both tables are zeros), prm1 [M][DP][mu_x, 1/vx], prm4 [M][DP][mu_x, a, mu_y, q], cm[m] = c_m - D log 2 pi.
template <int LONLY, int FB>
__global__ void __launch_bounds__(kEmBdThreads)
traj_em_bd_kernel(const TrajUtt *__restrict__ utts, const EmBdJob *__restrict__ jobs, int D2, int DP, int M,
                  const double *__restrict__ prm1, const double *__restrict__ prm4, const double *__restrict__ cst,
                  const double *__restrict__ cm, double *__restrict__ lse_all, double *__restrict__ qbar_all,
                  double *__restrict__ gbar_all) {
  extern __shared__ double lds[];
  constexpr int RS = FB + 1, NS = 64 / FB, NW = kEmBdThreads / 64;
  double *xs = lds;                               // [DP][RS]
  double *ys = xs + (size_t)DP * RS;              // [DP][RS]
  double *L = ys + (size_t)DP * RS;               // [M][FB]
  double *red = L + (size_t)M * FB;               // [NP][FB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = lane & (FB - 1), sub = lane / FB;
  const EmBdJob J = jobs[blockIdx.x];
  const TrajUtt U = utts[J.utt];
  const int T = U.T, t0 = J.t0, D = D2 >> 1;
  const int nf = (T - t0 < FB) ? T - t0 : FB;
  const gdouble *X = (const gdouble *)U.X, *Yg = (const gdouble *)U.Y;

  // stage: rows beyond the utterance and beyond 2D are zeros on both sides
  for (int i = tid; i < FB * DP; i += kEmBdThreads) {
    const int fr = i / DP, k = i - fr * DP, t = t0 + fr;
    double x = 0.0, y = 0.0;
    if (fr < nf && k < D2) {
      x = X[(size_t)t * D2 + k];
      if (k < D) {
        y = Yg[(size_t)t * D + k];
      } else {
        const int d = k - D;
        const double yp = (t + 1 < T) ? Yg[(size_t)(t + 1) * D + d] : 0.0, ym = (t >= 1) ? Yg[(size_t)(t - 1) * D + d] : 0.0;
        y = 0.5 * yp - 0.5 * ym;
      }
    }
    xs[k * RS + fr] = x;
    ys[k * RS + fr] = y;
  }
  __syncthreads();

  // phase 1a: the source term, as bdmap_kernel's phase 1
  for (int mw = 4 * NS * wave; mw < M; mw += 4 * NS * NW) {
    int mb = mw + 4 * sub;
    if (FB == 64) mb = __builtin_amdgcn_readfirstlane(mb);
    const double *p[4];
    double q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = prm1 + (size_t)((mb + j < M) ? mb + j : M - 1) * DP * kBdmapPrm1;
    for (int k0 = 0; k0 < DP; k0 += 4) {
      double x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = xs[(k0 + k) * RS + f];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double *pj = p[j] + k0 * kBdmapPrm1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double dx = x[k] - pj[2 * k];
          q[j] = fma(dx * dx, pj[2 * k + 1], q[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (mb + j < M) L[(mb + j) * FB + f] = cst[mb + j] - 0.5 * q[j];
  }
  __syncthreads();

  // phase 2a: lse_m l of this thread's frame (tid & (FB - 1) == f: the frame of phase 1b's lane)
  const int part = tid / FB;
  const double lsx = em_bd_lse<FB, false>(L, red, M, f, part);

  // phase 1b: the target term; L <- (l - lse_m l) + (c_m - D log 2 pi - 1/2 sum_k q (Y - E)^2)
  for (int mw = 4 * NS * wave; mw < M; mw += 4 * NS * NW) {
    int mb = mw + 4 * sub;
    if (FB == 64) mb = __builtin_amdgcn_readfirstlane(mb);
    const double *p[4];
    double q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = prm4 + (size_t)((mb + j < M) ? mb + j : M - 1) * DP * kBdmapPrm4;
    for (int k0 = 0; k0 < DP; k0 += 2) {
      const double x0 = xs[k0 * RS + f], x1 = xs[(k0 + 1) * RS + f], y0 = ys[k0 * RS + f], y1 = ys[(k0 + 1) * RS + f];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double *pj = p[j] + k0 * kBdmapPrm4;
        const double e0 = y0 - fma(pj[1], x0 - pj[0], pj[2]);
        q[j] = fma(e0 * e0, pj[3], q[j]);
        const double e1 = y1 - fma(pj[5], x1 - pj[4], pj[6]);
        q[j] = fma(e1 * e1, pj[7], q[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (mb + j < M) L[(mb + j) * FB + f] = (L[(mb + j) * FB + f] - lsx) + (cm[mb + j] - 0.5 * q[j]);
  }
  __syncthreads();

  // phase 2b
  const double lse = em_bd_lse<FB, !LONLY>(L, red, M, f, part);
  if (part == 0 && f < nf) lse_all[U.frame0 + t0 + f] = lse;
  if (LONLY) return;
  __syncthreads();

  // phase 3: qbar and gbar of two features over all mixtures
  for (int kw = 2 * NS * wave; kw < DP; kw += 2 * NS * NW) {
    int kb = kw + 2 * sub;
    if (FB == 64) kb = __builtin_amdgcn_readfirstlane(kb);
    if (kb < DP) {
      const double x0 = xs[kb * RS + f], x1 = xs[(kb + 1) * RS + f];
      double qb0 = 0.0, qb1 = 0.0, gb0 = 0.0, gb1 = 0.0;
      const double *pp = prm4 + (size_t)kb * kBdmapPrm4;
#pragma unroll 2
      for (int m = 0; m < M; ++m) {
        const double g = L[m * FB + f];
        const double *r = pp + (size_t)m * DP * kBdmapPrm4;       // [mu_x, a, mu_y, q] of the two features
        qb0 = fma(g, r[3], qb0);
        gb0 = fma(g * r[3], fma(r[1], x0 - r[0], r[2]), gb0);
        qb1 = fma(g, r[7], qb1);
        gb1 = fma(g * r[7], fma(r[5], x1 - r[4], r[6]), gb1);
      }
      ys[kb * RS + f] = qb0;
      ys[(kb + 1) * RS + f] = qb1;
      xs[kb * RS + f] = gb0;
      xs[(kb + 1) * RS + f] = gb1;
    }
  }
  __syncthreads();

  // store: consecutive lanes on consecutive addresses
  const size_t F0 = (size_t)(U.frame0 + t0);
  for (int i = tid; i < FB * DP; i += kEmBdThreads) {
    const int fr = i / DP, k = i - fr * DP;
    if (fr < nf && k < D2) {
      qbar_all[(F0 + fr) * D2 + k] = ys[k * RS + fr];
      gbar_all[(F0 + fr) * D2 + k] = xs[k * RS + fr];
    }
  }
}

// the identity index of the EM loop's precision table: mh[f] = f + 1 over the packed frames
__global__ void __launch_bounds__(256)
traj_em_bd_index_kernel(int64_t *__restrict__ mh, int64_t nframes) {
  const int64_t fr = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (fr < nframes) mh[fr] = fr + 1;
}

// ---- host side ------------------------------------------------------------------------------------------------------
template <int LONLY, int FB>
static int em_bd_launch(const vcmi_traj *t, const TrajUtt *du, const EmBdJob *dj, int64_t njobs, double *lse, double *qbar,
                        double *gbar, hipStream_t st) {
  static std::atomic<bool> attr_done[64];
  const vcmi_bdmap *b = t->b;
  VCMI_TRY(set_max_dynamic_lds(traj_em_bd_kernel<LONLY, FB>, FB == 64 ? kEmBdLdsBudget : em_bd_lds_bytes(kEmBdMaxDP, kEmBdMaxM, 32),
                               attr_done));
  hipLaunchKernelGGL((traj_em_bd_kernel<LONLY, FB>), dim3((unsigned)njobs), dim3(kEmBdThreads), em_bd_lds_bytes(b->DP, b->M, FB), st,
                     du, dj, b->D, b->DP, b->M, b->prm1.p, b->prm4.p, b->cst.p, t->cm.p, lse, qbar, gbar);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// One fused pass over the jobs dj[0 .. njobs) of the (uploaded) utterances du at the y in their Y matrices: lse, and unless
// lonly the qbar table and gbar.  Asynchronous on st.
static int em_bd_pass(const vcmi_traj *t, const TrajUtt *du, const EmBdJob *dj, int64_t njobs, bool lonly, double *lse, double *qbar,
                      double *gbar, hipStream_t st) {
  if (njobs == 0) return VCMI_OK;
  if (em_bd_frames(t->b->DP, t->b->M) == 64)
    return lonly ? em_bd_launch<1, 64>(t, du, dj, njobs, lse, qbar, gbar, st) : em_bd_launch<0, 64>(t, du, dj, njobs, lse, qbar, gbar, st);
  return lonly ? em_bd_launch<1, 32>(t, du, dj, njobs, lse, qbar, gbar, st) : em_bd_launch<0, 32>(t, du, dj, njobs, lse, qbar, gbar, st);
}

// cm[m] = 1/2 sum_k log q_km - D log 2 pi on the handle, once (the sum over k ascending with a compensated accumulator, as
// BdmapTable::cst); the device the handle was made on
static int em_bd_ensure(vcmi_traj *t) {
  if (t->cm.p) return VCMI_OK;
  int dev = 0;
  VCMI_HIP(hipGetDevice(&dev));
  if (dev != t->b->device)
    return fail(VCMI_ERR_ARG, "vcmi_traj_set_em_bdiag: the handle was created on device %d, the call runs on device %d", t->b->device, dev);
  const int D2 = t->D2, M = t->M;
  const double log2pi = 1.8378770664093454835606594728112;
  std::vector<double> cm((size_t)M);
  for (int m = 0; m < M; ++m) {
    double s = 0.0, comp = 0.0;
    for (int k = 0; k < D2; ++k) {
      const double lv = std::log(t->b->h_q[(size_t)m * D2 + k]), tt = s + lv;
      comp += (std::fabs(s) >= std::fabs(lv)) ? (s - tt) + lv : (lv - tt) + s;
      s = tt;
    }
    cm[(size_t)m] = 0.5 * (s + comp) - t->D * log2pi;
  }
  return upload_now(t->cm, cm);
}

// the tile jobs of the utterances (in the order of their uploaded descriptors) on the device, in t->em_jobs
static int em_bd_upload_jobs(vcmi_traj *t, const std::vector<TrajUtt> &utts, int64_t *njobs) {
  std::vector<int32_t> T(utts.size());
  for (size_t u = 0; u < utts.size(); ++u) T[u] = utts[u].T;
  std::vector<EmBdJob> jobs;
  em_bd_jobs(T.data(), (int)T.size(), em_bd_frames(t->b->DP, t->b->M), &jobs);
  *njobs = (int64_t)jobs.size();
  if (jobs.empty()) return VCMI_OK;
  VCMI_TRY(t->em_jobs.reserve(2 * jobs.size()));
  return upload_now(t->em_jobs.p, jobs.data(), jobs.size() * sizeof(EmBdJob));
}

int traj_em_bdiag_run(vcmi_traj *t, const std::vector<TrajUtt> &utts, const TrajSolvePlan &plan, hipStream_t st) {
  const int n = plan.n, iters = t->em_iters, D2 = t->D2;
  const int64_t nframes = plan.nframes;
  if (!em_bd_frames_ok(nframes))
    return fail(VCMI_ERR_DIM, "BlockDiagTrajectoryEMGMMMap: %lld frames in one call exceed the EM loop's frame index", (long long)nframes);
  VCMI_TRY(em_bd_ensure(t));
  VCMI_TRY(t->em_table.reserve((size_t)em_bd_qbar_doubles(nframes, D2)));
  VCMI_TRY(t->em_lse.reserve((size_t)em_bd_lse_doubles(nframes)));
  VCMI_TRY(t->em_mh.reserve((size_t)em_bd_index_words(nframes)));
  VCMI_TRY(t->em_L.reserve((size_t)em_bd_L_doubles(iters, n)));
  int64_t njobs = 0;
  VCMI_TRY(em_bd_upload_jobs(t, utts, &njobs));
  const EmBdJob *dj = reinterpret_cast<const EmBdJob *>(t->em_jobs.p);
  hipLaunchKernelGGL(traj_em_bd_index_kernel, dim3((unsigned)((nframes + 255) / 256)), dim3(256), 0, st, t->em_mh.p, nframes);
  VCMI_HIP(hipGetLastError());
  for (int it = 0; it < iters; ++it) {
    VCMI_TRY(em_bd_pass(t, plan.du, dj, njobs, false, t->em_lse.p, t->em_table.p, t->gbuf.p, st));
    VCMI_TRY(traj_em_sum_launch(plan.du, n, t->em_lse.p, t->em_L.p + (size_t)it * n, st));
    VCMI_TRY(traj_band_solve_launch(t, plan, t->em_table.p, t->em_mh.p, st));
  }
  t->em_run_iters = iters;
  t->em_run_n = n;
  return VCMI_OK;
}

// the descriptor and the jobs of ONE utterance on the device (the buffers are shared with the conversion entries: st has been
// waited for)
static int em_bd_single(vcmi_traj *t, const double *dX, const double *dY, int64_t T, int64_t *njobs) {
  std::vector<TrajUtt> utts(1, TrajUtt{dX, const_cast<double *>(dY), 0, (int32_t)T, 0});
  VCMI_TRY(t->uttbuf.reserve(sizeof(TrajUtt)));
  VCMI_TRY(upload_now(t->uttbuf.p, utts.data(), sizeof(TrajUtt)));
  return em_bd_upload_jobs(t, utts, njobs);
}

static int em_bd_handle_check(const vcmi_traj *t, const char *who) {
  if (!t) return fail(VCMI_ERR_ARG, "%s: NULL handle", who);
  if (!t->b)
    return fail(VCMI_ERR_ARG, "%s: the converter was not made from a cross-diagonal model (vcmi_traj_create_bdiag); EM over a dense "
                              "model: vcmi_traj_set_em, vcmi_traj_cond_loglik", who);
  return VCMI_OK;
}

}  // namespace vcmi

using namespace vcmi;

extern "C" int vcmi_traj_set_em_bdiag(vcmi_traj *t, int iters) {
  VCMI_TRY(em_bd_handle_check(t, "vcmi_traj_set_em_bdiag"));
  if (iters < 0) return fail(VCMI_ERR_ARG, "vcmi_traj_set_em_bdiag: negative iteration count");
  if (iters > 0) VCMI_TRY(traj_two_windows_only(t, "vcmi_traj_set_em_bdiag", "EM re-estimation"));     // (the E-step's W is the two-window stencil)
  if (iters > 0) VCMI_TRY(em_bd_ensure(t));
  t->em_iters = iters;
  return VCMI_OK;
}

extern "C" int vcmi_traj_cond_loglik_bdiag_dev(vcmi_traj *t, const double *dX, const double *dY, int64_t T, double *dL, void *stream) {
  VCMI_TRY(em_bd_handle_check(t, "vcmi_traj_cond_loglik_bdiag_dev"));
  VCMI_TRY(traj_two_windows_only(t, "vcmi_traj_cond_loglik_bdiag_dev", "L(y)"));
  if (!dL) return fail(VCMI_ERR_ARG, "vcmi_traj_cond_loglik_bdiag_dev: NULL argument");
  if (T < 0 || T > INT32_MAX || (T > 0 && (!dX || !dY))) return fail(VCMI_ERR_ARG, "vcmi_traj_cond_loglik_bdiag_dev: bad argument");
  hipStream_t st = as_stream(stream);
  if (T == 0) {
    VCMI_HIP(hipMemsetAsync(dL, 0, sizeof(double), st));
    return VCMI_OK;
  }
  VCMI_TRY(em_bd_ensure(t));
  VCMI_TRY(t->em_lse.reserve((size_t)T));
  VCMI_HIP(hipStreamSynchronize(st));       // (the descriptor buffer is shared with the conversion calls)
  int64_t njobs = 0;
  VCMI_TRY(em_bd_single(t, dX, dY, T, &njobs));
  const TrajUtt *du = reinterpret_cast<const TrajUtt *>(t->uttbuf.p);
  VCMI_TRY(em_bd_pass(t, du, reinterpret_cast<const EmBdJob *>(t->em_jobs.p), njobs, true, t->em_lse.p, nullptr, nullptr, st));
  return traj_em_sum_launch(du, 1, t->em_lse.p, dL, st);
}

extern "C" int vcmi_traj_cond_loglik_bdiag(vcmi_traj *t, const double *X, const double *Y, int64_t T, double *L) {
  VCMI_TRY(em_bd_handle_check(t, "vcmi_traj_cond_loglik_bdiag"));
  VCMI_TRY(traj_two_windows_only(t, "vcmi_traj_cond_loglik_bdiag", "L(y)"));
  if (!L) return fail(VCMI_ERR_ARG, "vcmi_traj_cond_loglik_bdiag: NULL argument");
  if (T < 0 || T > INT32_MAX || (T > 0 && (!X || !Y))) return fail(VCMI_ERR_ARG, "vcmi_traj_cond_loglik_bdiag: bad argument");
  *L = 0.0;
  if (T == 0) return VCMI_OK;
  VCMI_TRY(t->xbuf.reserve((size_t)T * t->D2));
  VCMI_TRY(t->ybuf.reserve((size_t)T * t->D + 1));
  VCMI_TRY(upload_now(t->xbuf.p, X, sizeof(double) * T * t->D2));
  VCMI_TRY(upload_now(t->ybuf.p, Y, sizeof(double) * T * t->D));
  double *dL = t->ybuf.p + (size_t)T * t->D;
  VCMI_TRY(vcmi_traj_cond_loglik_bdiag_dev(t, t->xbuf.p, t->ybuf.p, T, dL, nullptr));
  VCMI_HIP(hipStreamSynchronize(nullptr));
  VCMI_HIP(hipMemcpy(L, dL, sizeof(double), hipMemcpyDeviceToHost));
  traj_em_release(t);
  return VCMI_OK;
}

// Test hook (not part of include/vcmi.h; tests/test_gpu_traj_em_bdiag.py): one fused pass at a caller-given y for one utterance,
// host pointers X (2D,T), Y (D,T) -> lse (T), qbar (2D,T), gbar (2D,T).
extern "C" int vcmi_debug_traj_em_bdiag_estep(vcmi_traj *t, const double *X, const double *Y, int64_t T, double *lse, double *qbar,
                                              double *gbar) {
  VCMI_TRY(em_bd_handle_check(t, "vcmi_debug_traj_em_bdiag_estep"));
  VCMI_TRY(traj_two_windows_only(t, "vcmi_debug_traj_em_bdiag_estep", "the E-step"));
  if (T < 0 || T > INT32_MAX - 1 || (T > 0 && (!X || !Y || !lse || !qbar || !gbar)))
    return fail(VCMI_ERR_ARG, "vcmi_debug_traj_em_bdiag_estep: bad argument");
  if (T == 0) return VCMI_OK;
  const size_t nx = (size_t)T * t->D2;
  VCMI_TRY(em_bd_ensure(t));
  VCMI_TRY(t->xbuf.reserve(nx));
  VCMI_TRY(t->ybuf.reserve((size_t)T * t->D));
  VCMI_TRY(t->gbuf.reserve(nx));
  VCMI_TRY(t->em_table.reserve(nx));
  VCMI_TRY(t->em_lse.reserve((size_t)T));
  VCMI_HIP(hipStreamSynchronize(nullptr));
  VCMI_TRY(upload_now(t->xbuf.p, X, sizeof(double) * nx));
  VCMI_TRY(upload_now(t->ybuf.p, Y, sizeof(double) * T * t->D));
  int64_t njobs = 0;
  VCMI_TRY(em_bd_single(t, t->xbuf.p, t->ybuf.p, T, &njobs));
  VCMI_TRY(em_bd_pass(t, reinterpret_cast<const TrajUtt *>(t->uttbuf.p), reinterpret_cast<const EmBdJob *>(t->em_jobs.p), njobs, false,
                      t->em_lse.p, t->em_table.p, t->gbuf.p, nullptr));
  VCMI_HIP(hipStreamSynchronize(nullptr));
  VCMI_HIP(hipMemcpy(lse, t->em_lse.p, sizeof(double) * T, hipMemcpyDeviceToHost));
  VCMI_HIP(hipMemcpy(qbar, t->em_table.p, sizeof(double) * nx, hipMemcpyDeviceToHost));
  VCMI_HIP(hipMemcpy(gbar, t->gbuf.p, sizeof(double) * nx, hipMemcpyDeviceToHost));
  traj_em_release(t);
  return VCMI_OK;
}
