// traj_em.hip -- EM re-estimation of the trajectory over ALL mixtures (Toda, Black, Tokuda 2007, eqs. 30-36) in place of the
// suboptimum mixture sequence of src/trajectory_gmmmap.jl:81-82 (their eq. 37).  The kernels, the loop (traj_internal.hpp:
// traj_em_run) and the EM entries.
//
// Statement (restated in numpy in tests/traj_em_restatement.py).  Notation of traj.hip:9-17, every array unsymmetrised as the
// handle holds it:  Q_m = Dy_m,  E_{m,t} = b_m + A_m X_t,  pi_{m,t} = P(m | X_t) (src/gmm.jl:24-30; w_m <= 0 excluded),
// Y_t(y) = (W y)_t = [y_t ; (y_{t+1} - y_{t-1}) / 2] with W's boundary rule (a missing neighbour is dropped),
// c_m = logdet((Q_m + Q_m') / 2) / 2.
//   E-step   l_{m,t} = log pi_{m,t} + c_m - (Y_t - E_{m,t})' Q_m (Y_t - E_{m,t}) / 2 - D log 2 pi
//            lse_t = logsumexp_m l_{m,t} (max-shifted),  gamma_{m,t} = exp(l_{m,t} - lse_t),  L(y) = sum_t lse_t = log P(W y | X)
//   M-step   Qbar_t = sum_m gamma_{m,t} Q_m,  gbar_t = sum_m gamma_{m,t} Q_m E_{m,t};  the block-pentadiagonal system of traj.hip
//            with (Qbar_t, gbar_t) in place of (Q_mhat_t, g_t)
// y^0 is the arg-max solution; em_iters = n runs n E/M pairs.
//
// Kernels.  traj_em_post_kernel: 64 frames (four 16-frame tiles) of one utterance per workgroup, wave i owns row tile i of both
// products, all M mixtures in turn: e = Y_t - b_m - A_m X_t and v = Q_m e on v_mfma_f64_16x16x4 from the Afrag / Qfrag images
// (the chaining of traj_g_mfma_kernel), q = e . v per frame column, l, then gamma, lse and the pure / mixed flag per frame.
// traj_em_g_kernel: the same tiling, gbar_t over the mixtures some frame of the workgroup gives weight.  traj_em_valu_kernel:
// both for feature dimensions without fragments (NT > 6), one workgroup per frame like traj_g_kernel.  traj_em_scan_kernel
// compacts the mixed frames, traj_em_blend_kernel writes their Qbar_t behind the model's M matrices in one table.
#include "traj_internal.hpp"
#include "hostpipe.hpp"
#include "postf.hpp"

#include <algorithm>
#include <functional>

namespace vcmi {

static constexpr int kEmNB = 4;              // 16-frame tiles per workgroup of the MFMA kernels
static constexpr int kEmF = 16 * kEmNB;      // ... frames

// (W y)_t, row `row` of [static ; delta]
__device__ __forceinline__ double em_stencil(const double *__restrict__ y, int D, int T, int t, int row) {
  if (row < D) return y[(size_t)t * D + row];
  const int d = row - D;
  const double yp = (t + 1 < T) ? y[(size_t)(t + 1) * D + d] : 0.0, ym = (t >= 1) ? y[(size_t)(t - 1) * D + d] : 0.0;
  return 0.5 * yp - 0.5 * ym;
}

// sign * x of the workgroup's frames into LDS, k-major per 16-frame tile ([kEmNB][4 KS][16]); zero beyond T and beyond 2D
__device__ __forceinline__ void em_load_x(double *Xs, const double *__restrict__ X, int D2, int KS, int T, int t0, double sign) {
  const int per = 4 * KS * 16;
  for (int e = threadIdx.x; e < kEmNB * per; e += blockDim.x) {
    const int b = e / per, q = e - b * per, k = q >> 4, t = t0 + b * 16 + (q & 15);
    Xs[e] = (t < T && k < D2) ? sign * X[(size_t)t * D2 + k] : 0.0;
  }
}

// log w_m N(x_t) (T,M) -> log pi_{m,t} in place: one thread per frame (once per call; the rows are M doubles)
__global__ void __launch_bounds__(256)
traj_em_logprior_kernel(double *__restrict__ LP, int M, int64_t nframes) {
  const int64_t fr = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (fr >= nframes) return;
  double *l = LP + fr * M;
  double mx = -INFINITY;
  for (int m = 0; m < M; ++m) mx = fmax(mx, l[m]);
  double s = 0.0;
  for (int m = 0; m < M; ++m) s += exp(l[m] - mx);
  const double lse = mx + log(s);
  for (int m = 0; m < M; ++m) l[m] -= lse;
}

// l_{m,.} of one frame (written by the calling thread itself) -> gamma, lse, flag.  A frame is PURE when the COMPUTED
// 1 - exp(mx - lse) is below 2^-53: it takes that mixture alone (gamma written one-hot, flag = its index); otherwise MIXED
// (flag -1).  That is not "1 - max gamma < 2^-53": with r = sum_{m != best} exp(l_m - l_best) the weight dropped is r / (1 + r),
// but lse = mx + log(s) absorbs log(s) = log1p(r) as soon as it is below half an ulp of mx, and then exp(mx - lse) is exactly 1.
// So the line sits at r of about max(1, |l_best|) 2^-53 (up to 2^-52 |l_best| where |l_best| is just above a power of two), not at
// 2^-53: a frame is certainly mixed from r = 8 max(1, |l_best|) 2^-53 on and certainly pure up to r = 2^-56, either in between
// -- the dropped weight is then at most 8 |l_best| 2^-53, which the solver's operands do not see.  Pinned by
// tests/test_gpu_traj_em_terms.py::test_decision_line (band derived in tests/traj_em_restatement.py, "THE FLAG BAND").
__device__ __forceinline__ void em_finish_frame(double *__restrict__ gl, int M, double *__restrict__ lse_out, int *__restrict__ pure_out) {
  double mx = -INFINITY;
  int mi = 0;
  for (int m = 0; m < M; ++m) {
    const double v = gl[m];
    if (v > mx) {
      mx = v;
      mi = m;
    }
  }
  double s = 0.0;
  for (int m = 0; m < M; ++m) s += exp(gl[m] - mx);
  const double lse = mx + log(s);
  const bool pure = 1.0 - exp(mx - lse) < 0x1p-53;
  for (int m = 0; m < M; ++m) gl[m] = pure ? (m == mi ? 1.0 : 0.0) : exp(gl[m] - lse);
  *lse_out = lse;
  *pure_out = pure ? mi : -1;
}

typedef double em_d4 __attribute__((ext_vector_type(4)));
static constexpr int kEmMaxKS = 24;   // k-steps of the widest feature vector with fragments (2D <= 96)

// E-step.  grid (ceil(Tmax / 64), utterances), 64 NT threads; LDS: -x [kEmNB][4 KS][16], e in B-operand order [kEmNB][4 NT][64],
// q partials [NT][64].  4 M (2D)^2 flop per frame.
__global__ void __launch_bounds__(384)
traj_em_post_kernel(const TrajUtt *__restrict__ utts, int D2, int M, int KS, const double *__restrict__ Afrag,
                    const double *__restrict__ Qfrag, const double *__restrict__ bvec, const double *__restrict__ cm,
                    const double *__restrict__ lp_all, double *__restrict__ gam_all, double *__restrict__ lse_all,
                    int *__restrict__ pure_all) {
  extern __shared__ double esm[];
  const int nthr = blockDim.x, NT = nthr >> 6, D = D2 >> 1;
  double *Xn = esm;                                   // [kEmNB][4*KS][16]
  double *Ef = Xn + (size_t)kEmNB * 4 * KS * 16;      // [kEmNB][4*NT][64]
  double *qp = Ef + (size_t)kEmNB * 4 * NT * 64;      // [NT][kEmF]
  const TrajUtt U = utts[blockIdx.y];
  const int T = U.T, t0 = (int)blockIdx.x * kEmF;
  if (t0 >= T) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lcol = lane & 15, lgrp = lane >> 4;
  em_load_x(Xn, U.X, D2, KS, T, t0, -1.0);
  double ur[kEmNB][4];                                // Y_t = (W y)_t in accumulator layout, formed from y by the stencil
#pragma unroll
  for (int b = 0; b < kEmNB; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wave + lgrp + 4 * r, t = t0 + 16 * b + lcol;
      ur[b][r] = (row < D2 && t < T) ? em_stencil(U.Y, D, T, t, row) : 0.0;
    }
  double *gl = gam_all + (size_t)(U.frame0 + t0 + tid) * M;     // this thread's frame (tid < kEmF)
  const double *lp = lp_all + (size_t)(U.frame0 + t0 + tid) * M;
  const bool owner = tid < kEmF && t0 + tid < T;
  __syncthreads();
  for (int m = 0; m < M; ++m) {
    double afr[kEmMaxKS], qfr[kEmMaxKS];
    const double *A = Afrag + (((size_t)m * NT + wave) * KS) * 64 + lane;
    const double *Q = Qfrag + (((size_t)m * NT + wave) * KS) * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < kEmMaxKS; ++ks) {
      afr[ks] = (ks < KS) ? A[(size_t)ks * 64] : 0.0;
      qfr[ks] = (ks < KS) ? Q[(size_t)ks * 64] : 0.0;
    }
    double bm[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wave + lgrp + 4 * r;
      bm[r] = (row < D2) ? bvec[(size_t)m * D2 + row] : 0.0;
    }
    em_d4 er[kEmNB];
#pragma unroll
    for (int b = 0; b < kEmNB; ++b) {
      em_d4 acc;                                       // e = Y_t - b_m - A_m X_t
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = ur[b][r] - bm[r];
      const double *Xb = Xn + (size_t)b * 4 * KS * 16;
#pragma unroll
      for (int ks = 0; ks < kEmMaxKS; ++ks)
        if (ks < KS) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[ks], Xb[(4 * ks + lgrp) * 16 + lcol], acc, 0, 0, 0);
      er[b] = acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) Ef[((size_t)b * 4 * NT + 4 * wave + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < kEmNB; ++b) {
      em_d4 v = {0.0, 0.0, 0.0, 0.0};                  // v = Q_m e
      const double *Eb = Ef + (size_t)b * 4 * NT * 64;
#pragma unroll
      for (int ks = 0; ks < kEmMaxKS; ++ks)
        if (ks < KS) v = __builtin_amdgcn_mfma_f64_16x16x4f64(qfr[ks], Eb[(size_t)ks * 64 + lane], v, 0, 0, 0);
      double part = 0.0;                               // q = e . v of frame column lcol: this lane's four rows, then the lane groups
#pragma unroll
      for (int r = 0; r < 4; ++r) part = fma(er[b][r], v[r], part);
      part += __shfl_xor(part, 16);
      part += __shfl_xor(part, 32);
      if (lgrp == 0) qp[wave * kEmF + 16 * b + lcol] = part;
    }
    __syncthreads();
    if (owner) {
      double q = 0.0;
      for (int w = 0; w < NT; ++w) q += qp[w * kEmF + tid];
      gl[m] = lp[m] + cm[m] - 0.5 * q;
    }
  }
  if (owner) em_finish_frame(gl, M, lse_all + U.frame0 + t0 + tid, pure_all + U.frame0 + t0 + tid);
}

// gbar_t = sum_m gamma_{m,t} Q_m (b_m + A_m X_t) for the same 64 frames; a mixture that no frame of the workgroup gives weight
// (gamma exactly 0: every mixture but one on a pure frame) is skipped.  LDS: x, E in B-operand order, need [M].
__global__ void __launch_bounds__(384)
traj_em_g_kernel(const TrajUtt *__restrict__ utts, int D2, int M, int KS, const double *__restrict__ Afrag,
                 const double *__restrict__ Qfrag, const double *__restrict__ bvec, const double *__restrict__ gam_all,
                 double *__restrict__ G_all) {
  extern __shared__ double esm[];
  const int nthr = blockDim.x, NT = nthr >> 6;
  double *Xp = esm;                                   // [kEmNB][4*KS][16]
  double *Ef = Xp + (size_t)kEmNB * 4 * KS * 16;      // [kEmNB][4*NT][64]
  int *need = reinterpret_cast<int *>(Ef + (size_t)kEmNB * 4 * NT * 64);   // [M]
  const TrajUtt U = utts[blockIdx.y];
  const int T = U.T, t0 = (int)blockIdx.x * kEmF;
  if (t0 >= T) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lcol = lane & 15, lgrp = lane >> 4;
  const int nf = (T - t0 < kEmF) ? T - t0 : kEmF;
  const double *gam = gam_all + (size_t)(U.frame0 + t0) * M;
  for (int m = tid; m < M; m += nthr) need[m] = 0;
  em_load_x(Xp, U.X, D2, KS, T, t0, 1.0);
  __syncthreads();
  for (int e = tid; e < nf * M; e += nthr)
    if (gam[e] != 0.0) need[e % M] = 1;
  __syncthreads();
  em_d4 gacc[kEmNB];
#pragma unroll
  for (int b = 0; b < kEmNB; ++b) gacc[b] = em_d4{0.0, 0.0, 0.0, 0.0};
  for (int m = 0; m < M; ++m) {
    if (!need[m]) continue;                           // (workgroup-uniform)
    double afr[kEmMaxKS], qfr[kEmMaxKS];
    const double *A = Afrag + (((size_t)m * NT + wave) * KS) * 64 + lane;
    const double *Q = Qfrag + (((size_t)m * NT + wave) * KS) * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < kEmMaxKS; ++ks) {
      afr[ks] = (ks < KS) ? A[(size_t)ks * 64] : 0.0;
      qfr[ks] = (ks < KS) ? Q[(size_t)ks * 64] : 0.0;
    }
    double bm[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wave + lgrp + 4 * r;
      bm[r] = (row < D2) ? bvec[(size_t)m * D2 + row] : 0.0;
    }
#pragma unroll
    for (int b = 0; b < kEmNB; ++b) {
      em_d4 acc;                                       // E = b_m + A_m X_t, src/trajectory_gmmmap.jl:88
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = bm[r];
      const double *Xb = Xp + (size_t)b * 4 * KS * 16;
#pragma unroll
      for (int ks = 0; ks < kEmMaxKS; ++ks)
        if (ks < KS) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[ks], Xb[(4 * ks + lgrp) * 16 + lcol], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) Ef[((size_t)b * 4 * NT + 4 * wave + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < kEmNB; ++b) {
      em_d4 v = {0.0, 0.0, 0.0, 0.0};                  // Q_m E
      const double *Eb = Ef + (size_t)b * 4 * NT * 64;
#pragma unroll
      for (int ks = 0; ks < kEmMaxKS; ++ks)
        if (ks < KS) v = __builtin_amdgcn_mfma_f64_16x16x4f64(qfr[ks], Eb[(size_t)ks * 64 + lane], v, 0, 0, 0);
      const int f = 16 * b + lcol;
      const double wgt = (f < nf) ? gam[(size_t)f * M + m] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) gacc[b][r] = fma(wgt, v[r], gacc[b][r]);
    }
    __syncthreads();
  }
  double *G = G_all + (size_t)(U.frame0 + t0) * D2;
#pragma unroll
  for (int b = 0; b < kEmNB; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wave + lgrp + 4 * r, f = 16 * b + lcol;
      if (row < D2 && f < nf) G[(size_t)f * D2 + row] = gacc[b][r];
    }
}

// Both steps for feature dimensions without fragments (2D > 96): one workgroup (256 threads) per frame, thread r owns rows
// r, r + 256, ... (the style of traj_g_kernel).  LDS: x [D2], u [D2], e [D2], red [256], l [M], gbar [D2].  with_g = 0: E-step only.
__global__ void __launch_bounds__(256)
traj_em_valu_kernel(const TrajUtt *__restrict__ utts, int D2, int M, const double *__restrict__ AT, const double *__restrict__ QT,
                    const double *__restrict__ bvec, const double *__restrict__ cm, const double *__restrict__ lp_all,
                    double *__restrict__ gam_all, double *__restrict__ lse_all, int *__restrict__ pure_all,
                    double *__restrict__ G_all, int with_g) {
  extern __shared__ double vsm[];
  double *xs = vsm, *us = xs + D2, *es = us + D2, *red = es + D2, *ell = red + 256;
  const TrajUtt U = utts[blockIdx.y];
  const int T = U.T, t = (int)blockIdx.x, D = D2 >> 1, tid = threadIdx.x;
  if (t >= T) return;
  const int64_t fr = U.frame0 + t;
  for (int r = tid; r < D2; r += 256) {
    xs[r] = U.X[(size_t)t * D2 + r];
    us[r] = em_stencil(U.Y, D, T, t, r);
  }
  __syncthreads();
  for (int m = 0; m < M; ++m) {
    const double *A = AT + (size_t)m * D2 * D2, *Q = QT + (size_t)m * D2 * D2;
    for (int r = tid; r < D2; r += 256) {
      double e = us[r] - bvec[(size_t)m * D2 + r];
      for (int k = 0; k < D2; ++k) e = fma(-A[(size_t)k * D2 + r], xs[k], e);
      es[r] = e;
    }
    __syncthreads();
    double part = 0.0;
    for (int r = tid; r < D2; r += 256) {
      double v = 0.0;
      for (int k = 0; k < D2; ++k) v = fma(Q[(size_t)k * D2 + r], es[k], v);
      part = fma(es[r], v, part);
    }
    red[tid] = part;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) ell[m] = lp_all[fr * M + m] + cm[m] - 0.5 * red[0];
    __syncthreads();
  }
  if (tid == 0) em_finish_frame(ell, M, lse_all + fr, pure_all + fr);
  __syncthreads();
  for (int m = tid; m < M; m += 256) gam_all[fr * M + m] = ell[m];
  if (!with_g) return;
  double *gs = ell + M;                                // [D2] gbar of the frame; thread r owns rows r, r + 256, ...
  for (int r = tid; r < D2; r += 256) gs[r] = 0.0;
  for (int m = 0; m < M; ++m) {
    const double wgt = ell[m];
    if (wgt == 0.0) continue;                          // (workgroup-uniform)
    const double *A = AT + (size_t)m * D2 * D2, *Q = QT + (size_t)m * D2 * D2;
    __syncthreads();
    for (int r = tid; r < D2; r += 256) {
      double e = bvec[(size_t)m * D2 + r];
      for (int k = 0; k < D2; ++k) e = fma(A[(size_t)k * D2 + r], xs[k], e);
      es[r] = e;
    }
    __syncthreads();
    for (int r = tid; r < D2; r += 256) {
      double v = 0.0;
      for (int k = 0; k < D2; ++k) v = fma(Q[(size_t)k * D2 + r], es[k], v);
      gs[r] = fma(wgt, v, gs[r]);
    }
  }
  for (int r = tid; r < D2; r += 256) G_all[fr * D2 + r] = gs[r];
}

// L of every utterance: sum of lse over its frames in a fixed order (thread-strided partials, then a tree)
__global__ void __launch_bounds__(256)
traj_em_sum_kernel(const TrajUtt *__restrict__ utts, const double *__restrict__ lse_all, double *__restrict__ L) {
  __shared__ double red[256];
  const TrajUtt U = utts[blockIdx.x];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int t = tid; t < U.T; t += 256) s += lse_all[U.frame0 + t];
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) L[U.idx] = red[0];
}

// Scan of the flags over the utterances of a slice (one workgroup, 1024 threads): mh[t] = m + 1 for a pure frame, M + k + 1 for
// the k-th mixed frame (the solvers read table entry mh[t] - 1); mix[k] = its packed frame index; *count = mixed frames.
__global__ void __launch_bounds__(1024)
traj_em_scan_kernel(const TrajUtt *__restrict__ utts, int nu, int M, const int *__restrict__ pure_all, int64_t *__restrict__ mh_all,
                    int *__restrict__ mix, int *__restrict__ count) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int u = 0; u < nu; ++u) {
    const TrajUtt U = utts[u];
    for (int c0 = 0; c0 < U.T; c0 += 1024) {
      const int t = c0 + tid;
      const int p = (t < U.T) ? pure_all[U.frame0 + t] : 0;
      const bool mixed = t < U.T && p < 0;
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(mixed);
      const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
      if (lane == 0) wsum[wave] = __builtin_popcountll(mask);
      __syncthreads();
      int off = 0, total = 0;
      for (int w = 0; w < 16; ++w) {
        const int c = wsum[w];
        if (w < wave) off += c;
        total += c;
      }
      if (t < U.T) {
        const int k = base + off + rank;
        mh_all[U.frame0 + t] = mixed ? (int64_t)M + k + 1 : (int64_t)p + 1;
        if (mixed) mix[k] = (int)(U.frame0 + t);
      }
      base += total;
      __syncthreads();
    }
  }
  if (tid == 0) *count = base;
}

// Qbar of the mixed frames: [16 frames x M] . [M x E] on v_mfma_f64_16x16x4, E = (2 Ds)^2 elements of the table the solver
// reads (Q, or Qpad).  A operand: gamma of the tile's 16 frames, four mixtures per k-step; B operand: 16 consecutive elements
// of those four matrices.  grid (mixed tiles, element chunks), a wave per 16-element column block.  2 M E flop, E doubles
// written per frame.  Dp != 0: the table is Qpad, (2 Dp)^2 elements with static dimension D padded to Dp; the padding's unit
// diagonal is written as 1 -- the computed sum of gamma is 1 only to a few ulp (tests/test_gpu_traj_em_terms.py found
// 1 - 1.8e-15 there), and the padded solver's operands should not depend on the posteriors.
__global__ void __launch_bounds__(256)
traj_em_blend_kernel(const double *__restrict__ Qtab, int M, int64_t E, const double *__restrict__ gam_all,
                     const int *__restrict__ mix, int count, double *__restrict__ out, int D, int Dp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lcol = lane & 15, lgrp = lane >> 4;
  const int64_t k0 = (int64_t)blockIdx.x * 16;
  const int fr = (k0 + lcol < count) ? mix[k0 + lcol] : -1;
  const double *gam = gam_all + (size_t)(fr < 0 ? 0 : fr) * M;
  const int64_t ncb = (E + 15) / 16;
  const int KM = (M + 3) / 4;
  for (int64_t cb = (int64_t)blockIdx.y * 4 + wave; cb < ncb; cb += (int64_t)gridDim.y * 4) {
    const int64_t el = cb * 16 + lcol;
    em_d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int ks = 0; ks < KM; ++ks) {
      const int m = 4 * ks + lgrp;
      const double a = (fr >= 0 && m < M) ? gam[m] : 0.0;
      const double b = (m < M && el < E) ? Qtab[(size_t)m * E + el] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    const int64_t row = Dp ? el / (2 * Dp) : 0;
    const bool unit = Dp && row >= D && row < Dp && el == row * (2 * Dp) + row;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t k = k0 + lgrp + 4 * r;
      if (k < count && el < E) out[(size_t)k * E + el] = unit ? 1.0 : acc[r];
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// log pi_{m,t} of every frame of the call into em_lp (the weights come from X alone: once per call)
static int traj_em_prior(vcmi_traj *t, const std::vector<TrajUtt> &utts, int64_t nframes, bool contiguous, const double *dX0,
                         hipStream_t st) {
  const int D2 = t->D2, M = t->M;
  VCMI_TRY(t->em_lp.reserve((size_t)nframes * M));
  if (contiguous) {
    VCMI_TRY(gmmmap_logdens_device(t->g, dX0, D2, nframes, t->em_lp.p, st));
  } else {
    for (auto &u : utts)
      if (u.T > 0) VCMI_TRY(gmmmap_logdens_device(t->g, u.X, D2, u.T, t->em_lp.p + (size_t)u.frame0 * M, st));
  }
  hipLaunchKernelGGL(traj_em_logprior_kernel, dim3((unsigned)((nframes + 255) / 256)), dim3(256), 0, st, t->em_lp.p, M, nframes);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// E-step of the (uploaded) utterances du[0 .. nu) at the y in their Y matrices: gamma, lse and the flags; with_g: gbar into gbuf
// as well.  Tmax: their longest.
static int traj_em_estep(vcmi_traj *t, const TrajUtt *du, int nu, int Tmax, int64_t nframes, bool with_g, hipStream_t st,
                         hipEvent_t mid = nullptr) {
  const int D2 = t->D2, M = t->M;
  VCMI_TRY(t->em_gamma.reserve((size_t)nframes * M));
  VCMI_TRY(t->em_lse.reserve((size_t)nframes));
  VCMI_TRY(t->em_pure.reserve((size_t)nframes));
  if (t->NT <= 6 && !debug_flag(kDbgTrajGScalar)) {
    const int nthr = 64 * t->NT;
    const dim3 grid((unsigned)((Tmax + kEmF - 1) / kEmF), (unsigned)nu);
    const size_t tiles = ((size_t)kEmNB * 4 * t->KS * 16 + (size_t)kEmNB * 4 * t->NT * 64) * sizeof(double);
    const size_t shp = tiles + (size_t)t->NT * kEmF * sizeof(double), shg = tiles + (size_t)M * sizeof(int);
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(traj_em_post_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shp));
    hipLaunchKernelGGL(traj_em_post_kernel, grid, dim3(nthr), shp, st, du, D2, M, t->KS, t->Afrag.p, t->Qfrag.p, t->bvec.p, t->cm.p,
                       t->em_lp.p, t->em_gamma.p, t->em_lse.p, t->em_pure.p);
    if (mid) VCMI_HIP(hipEventRecord(mid, st));
    if (with_g) {
      VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(traj_em_g_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shg));
      hipLaunchKernelGGL(traj_em_g_kernel, grid, dim3(nthr), shg, st, du, D2, M, t->KS, t->Afrag.p, t->Qfrag.p, t->bvec.p,
                         t->em_gamma.p, t->gbuf.p);
    }
  } else {
    const size_t shv = ((size_t)4 * D2 + 256 + M) * sizeof(double);
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(traj_em_valu_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shv));
    hipLaunchKernelGGL(traj_em_valu_kernel, dim3((unsigned)Tmax, (unsigned)nu), dim3(256), shv, st, du, D2, M, t->AT.p, t->QT.p, t->bvec.p,
                       t->cm.p, t->em_lp.p, t->em_gamma.p, t->em_lse.p, t->em_pure.p, t->gbuf.p, with_g ? 1 : 0);
    if (mid) VCMI_HIP(hipEventRecord(mid, st));     // (one kernel does both: its time counts as E-step)
  }
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// Flag scan of the (uploaded) utterances du[0 .. nu), fs frames in all: em_mh, em_mix and the mixed-frame count, which is read
// back (the 4-byte read that synchronises st).  nframes: the frames of the call, behind which em_mix keeps the count.
static int traj_em_scan(vcmi_traj *t, const TrajUtt *du, int nu, int64_t nframes, int64_t fs, hipStream_t st, int *count) {
  int *dcount = t->em_mix.p + nframes;
  hipLaunchKernelGGL(traj_em_scan_kernel, dim3(1), dim3(1024), 0, st, du, nu, t->M, t->em_pure.p, t->em_mh.p, t->em_mix.p, dcount);
  VCMI_HIP(hipGetLastError());
  *count = 0;
  VCMI_HIP(hipMemcpyAsync(count, dcount, sizeof(int), hipMemcpyDeviceToHost, st));
  VCMI_HIP(hipStreamSynchronize(st));
  if (*count < 0 || *count > fs)
    return fail(VCMI_ERR_HIP, "TrajectoryGMMMap: EM flag scan returned %d mixed frames of %lld", *count, (long long)fs);
  return VCMI_OK;
}

// em_table = [the M matrices of the table the solver reads | Qbar of the count mixed frames]: t->Qpad in t->Dpad when padded,
// else t->Q
static int traj_em_blend(vcmi_traj *t, bool padded, int count, hipStream_t st) {
  const int M = t->M, Ds = padded ? t->Dpad : t->D;
  const int64_t E = (int64_t)4 * Ds * Ds;
  const double *Qsrc = padded ? t->Qpad.p : t->Q.p;
  VCMI_TRY(t->em_table.reserve((size_t)(M + count) * (size_t)E));
  VCMI_HIP(hipMemcpyAsync(t->em_table.p, Qsrc, sizeof(double) * (size_t)M * (size_t)E, hipMemcpyDeviceToDevice, st));
  if (count > 0) {
    const unsigned chunks = (unsigned)std::min<int64_t>(((E + 15) / 16 + 3) / 4, 8);
    hipLaunchKernelGGL(traj_em_blend_kernel, dim3((unsigned)((count + 15) / 16), chunks), dim3(256), 0, st, Qsrc, M, E, t->em_gamma.p,
                       t->em_mix.p, count, t->em_table.p + (size_t)M * (size_t)E, t->D, padded ? t->Dpad : 0);
    VCMI_HIP(hipGetLastError());
  }
  return VCMI_OK;
}

// em_iters E/M pairs after the arg-max solve of traj_run.  The table is sized by the mixed-frame count, one 4-byte read per
// iteration (the only host synchronisation of the loop); the batch (sorted, uploaded at du) starts as ONE slice and is cut into
// slices of whole utterances only where that count would take the table past kTrajEmTableCapBytes.
int traj_em_run(vcmi_traj *t, const std::vector<TrajUtt> &utts, const TrajSolvePlan &plan, bool contiguous, const double *dX0,
                hipStream_t st) {
  if (!t->em_pd) return fail(VCMI_ERR_NOT_PD, "TrajectoryGMMMap: EM needs (Q_m + Q_m')/2 positive definite");
  const int n = plan.n;
  const int64_t nframes = plan.nframes;
  const TrajUtt *du = plan.du;
  if (nframes > INT32_MAX) return fail(VCMI_ERR_DIM, "TrajectoryGMMMap: too many frames in one call for EM");
  const int M = t->M, iters = t->em_iters;
  const int64_t E = (int64_t)4 * plan.Ds * plan.Ds;
  VCMI_TRY(traj_em_prior(t, utts, nframes, contiguous, dX0, st));
  VCMI_TRY(t->em_mh.reserve((size_t)nframes));
  VCMI_TRY(t->em_mix.reserve((size_t)nframes + 1));
  VCMI_TRY(t->em_L.reserve((size_t)iters * n));
  struct Events {
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Events() {
      for (hipEvent_t x : e)
        if (x) (void)hipEventDestroy(x);
    }
    hipEvent_t &operator[](int k) { return e[k]; }
  } ev;
  if (t->em_time)
    for (int k = 0; k < 5; ++k) VCMI_HIP(hipEventCreate(&ev[k]));
  // iterations it0 .. iters-1 of the (sorted) utterances [b0, b0 + nb).  A slice whose table would pass the cap at some
  // iteration is cut in two there (by frames) and each half goes on from that iteration by itself: its E-step is repeated on
  // the same y, so the results do not depend on where the cuts fall.  One utterance is never cut.
  const size_t cap = t->em_cap_bytes ? t->em_cap_bytes : kTrajEmTableCapBytes;
  std::function<int(int, int, int)> run_slice = [&](int b0, int nb, int it0) -> int {
    const int Tmax = utts[(size_t)b0].T;                // (longest first)
    int64_t fs = 0;
    for (int u = 0; u < nb; ++u) fs += utts[(size_t)(b0 + u)].T;
    for (int it = it0; it < iters; ++it) {
      if (Tmax == 0) {                                  // only empty utterances: L = 0
        hipLaunchKernelGGL(traj_em_sum_kernel, dim3((unsigned)nb), dim3(256), 0, st, du + b0, t->em_lse.p, t->em_L.p + (size_t)it * n);
        continue;
      }
      if (t->em_time) VCMI_HIP(hipEventRecord(ev[0], st));
      VCMI_TRY(traj_em_estep(t, du + b0, nb, Tmax, nframes, true, st, t->em_time ? ev[1] : nullptr));
      if (t->em_time) VCMI_HIP(hipEventRecord(ev[2], st));
      hipLaunchKernelGGL(traj_em_sum_kernel, dim3((unsigned)nb), dim3(256), 0, st, du + b0, t->em_lse.p, t->em_L.p + (size_t)it * n);
      int count = 0;
      VCMI_TRY(traj_em_scan(t, du + b0, nb, nframes, fs, st, &count));
      const size_t table = (size_t)(M + count) * (size_t)E;
      if (table * sizeof(double) > cap && nb > 1) {
        int h = 0;
        for (int64_t f = 0; h < nb - 1 && 2 * f < fs; ++h) f += utts[(size_t)(b0 + h)].T;
        h = std::max(h, 1);
        VCMI_TRY(run_slice(b0, h, it));
        return run_slice(b0 + h, nb - h, it);
      }
      VCMI_TRY(traj_em_blend(t, plan.padded, count, st));
      if (t->em_time) VCMI_HIP(hipEventRecord(ev[3], st));
      VCMI_TRY(traj_solve_launch(t, plan, t->em_table.p, t->em_mh.p, b0, nb, st));
      if (t->em_time) {
        VCMI_HIP(hipEventRecord(ev[4], st));
        VCMI_HIP(hipEventSynchronize(ev[4]));
        float ms[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 4; ++k) VCMI_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
        EmTimes &m = t->em_times;
        m.estep_ms += ms[0];
        m.gbar_ms += ms[1];
        m.blend_ms += ms[2];
        m.solve_ms += ms[3];
        m.mixed_frames += count;
        m.frames += fs;
        m.table_bytes = std::max(m.table_bytes, table * sizeof(double));
        m.slices += 1;
      }
    }
    return VCMI_OK;
  };
  VCMI_TRY(run_slice(0, n, 0));
  t->em_run_iters = iters;
  t->em_run_n = n;
  return VCMI_OK;
}

int traj_em_sum_launch(const TrajUtt *du, int n, const double *lse, double *L, hipStream_t st) {
  hipLaunchKernelGGL(traj_em_sum_kernel, dim3((unsigned)n), dim3(256), 0, st, du, lse, L);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// the EM scratch of the handle in bytes: what the release rule weighs
static size_t traj_em_scratch_bytes(const vcmi_traj *t) {
  return (t->em_lp.n + t->em_gamma.n + t->em_lse.n + t->em_table.n + t->em_L.n + t->em_mh.n) * sizeof(double) +
         (t->em_pure.n + t->em_mix.n) * sizeof(int);
}

void traj_em_release(vcmi_traj *t) {
  if (traj_em_scratch_bytes(t) <= kVcScratchKeepBytes) return;
  t->em_lp.release();
  t->em_gamma.release();
  t->em_lse.release();
  t->em_table.release();
  t->em_L.release();
  t->em_mh.release();
  t->em_pure.release();
  t->em_mix.release();
}

TrajEmRelease::~TrajEmRelease() {
  if (!t->em_table.p && !t->em_gamma.p) return;
  if (traj_em_scratch_bytes(t) <= kVcScratchKeepBytes) return;
  (void)hipDeviceSynchronize();
  traj_em_release(t);
}

}  // namespace vcmi

using namespace vcmi;

// ---- EM re-estimation: the setting, the objective, the history -----------------------------------------------------------
extern "C" int vcmi_traj_set_em(vcmi_traj *t, int iters) {
  if (!t) return fail(VCMI_ERR_ARG, "vcmi_traj_set_em: NULL handle");
  if (iters < 0) return fail(VCMI_ERR_ARG, "vcmi_traj_set_em: negative iteration count");
  if (iters > 0 && t->precision == VCMI_TRAJ_PRECISION_DIAG)    // the M-step blends full precision matrices
    return fail(VCMI_ERR_ARG, "vcmi_traj_set_em: the converter has diagonal conditional precisions (vcmi_traj_set_precision)");
  if (iters > 0 && !t->em_pd)
    return fail(VCMI_ERR_NOT_PD, "vcmi_traj_set_em: (Q_m + Q_m')/2 of some mixture is not positive definite: the EM objective is undefined");
  t->em_iters = iters;
  return VCMI_OK;
}
extern "C" int vcmi_traj_get_em(const vcmi_traj *t) { return t ? t->em_iters : -1; }
// Measurement hook (not part of include/vcmi.h; tools/traj_em_bench.py): with enable != 0 the EM loop of this handle records hip
// events around its steps (and waits for them once per iteration).  out (8): ms of E-step, gbar, flag scan + count read + blend,
// pad + solve; mixed frames; largest table in bytes; frames; slice-iterations -- accumulated since the last call, which resets them.
extern "C" int vcmi_debug_traj_em_times(vcmi_traj *t, int enable, double *out) {
  if (!t) return fail(VCMI_ERR_ARG, "vcmi_debug_traj_em_times: NULL handle");
  const EmTimes &m = t->em_times;
  const double v[8] = {m.estep_ms, m.gbar_ms, m.blend_ms, m.solve_ms, (double)m.mixed_frames, (double)m.table_bytes, (double)m.frames,
                       (double)m.slices};
  for (int k = 0; out && k < 8; ++k) out[k] = v[k];
  t->em_times = EmTimes();
  t->em_time = enable != 0;
  return VCMI_OK;
}
// Test hook (not part of include/vcmi.h): the table cap of this handle's EM loop in bytes, so that the slicing can be tested
// on small inputs; 0 restores kTrajEmTableCapBytes.  (A setting of one handle: nothing process-wide.)
extern "C" int vcmi_debug_traj_em_cap(vcmi_traj *t, size_t bytes) {
  if (!t) return fail(VCMI_ERR_ARG, "vcmi_debug_traj_em_cap: NULL handle");
  t->em_cap_bytes = bytes;
  return VCMI_OK;
}

// Test hook (not part of include/vcmi.h; tests/test_gpu_traj_em_terms.py): what one iteration of the loop hands its solver, for
// one utterance at a caller-given y.  Host pointers X (2D,T), Y (D,T) -> gamma (M,T), lse (T), flag (T; the mixture of a pure
// frame, -1 for a mixed one), gbar (2D,T), mh (T; table index + 1), *count mixed frames and their blended matrices table
// (count of them, room for T; E = (2D)^2 elements each from t->Q, or with pad != 0 (2 Dpad)^2 from t->Qpad: the operands of the
// padded blocked solver).  Runs traj_em_prior, traj_em_estep (which honours DBG_TRAJ_G_SCALAR), traj_em_scan, traj_em_blend; the
// EM scratch follows traj_em_release's rule on every return.
extern "C" int vcmi_debug_traj_em_estep(vcmi_traj *t, const double *X, const double *Y, int64_t T, int pad, double *gamma, double *lse,
                                        int32_t *flag, double *gbar, int64_t *mh, int32_t *count, double *table) {
  if (!t || !count) return fail(VCMI_ERR_ARG, "vcmi_debug_traj_em_estep: NULL argument");
  if (t->b) return fail(VCMI_ERR_ARG, "vcmi_debug_traj_em_estep: the converter was made from a cross-diagonal model (vcmi_traj_create_bdiag)");
  if (t->precision == VCMI_TRAJ_PRECISION_DIAG)
    return fail(VCMI_ERR_ARG, "vcmi_debug_traj_em_estep: the converter has diagonal conditional precisions (vcmi_traj_set_precision)");
  if (!t->em_pd) return fail(VCMI_ERR_NOT_PD, "vcmi_debug_traj_em_estep: (Q_m + Q_m')/2 of some mixture is not positive definite");
  if (pad && !t->Dpad) return fail(VCMI_ERR_ARG, "vcmi_debug_traj_em_estep: the converter has no padded dimension");
  if (T < 0 || T > INT32_MAX - 1 || (T > 0 && (!X || !Y || !gamma || !lse || !flag || !gbar || !mh || !table)))
    return fail(VCMI_ERR_ARG, "vcmi_debug_traj_em_estep: bad argument");
  *count = 0;
  if (T == 0) return VCMI_OK;
  const int D2 = t->D2, M = t->M, Ds = pad ? t->Dpad : t->D;
  const int64_t E = (int64_t)4 * Ds * Ds;
  const size_t nx = (size_t)T * D2;
  hipStream_t st = nullptr;
  TrajEmRelease release{t};                 // the scratch rule on every way out, error returns included
  VCMI_TRY(t->xbuf.reserve(nx));
  VCMI_TRY(t->ybuf.reserve((size_t)T * t->D));
  VCMI_TRY(t->gbuf.reserve(nx));
  VCMI_TRY(t->uttbuf.reserve(sizeof(TrajUtt)));
  VCMI_TRY(t->em_mh.reserve((size_t)T));
  VCMI_TRY(t->em_mix.reserve((size_t)T + 1));
  VCMI_HIP(hipStreamSynchronize(st));       // (the buffers are shared with the conversion calls)
  VCMI_TRY(upload_now(t->xbuf.p, X, sizeof(double) * nx));
  VCMI_TRY(upload_now(t->ybuf.p, Y, sizeof(double) * T * t->D));
  std::vector<TrajUtt> utts(1, TrajUtt{t->xbuf.p, t->ybuf.p, 0, (int32_t)T, 0});
  VCMI_TRY(upload_now(t->uttbuf.p, utts.data(), sizeof(TrajUtt)));
  const TrajUtt *du = reinterpret_cast<const TrajUtt *>(t->uttbuf.p);
  VCMI_TRY(traj_em_prior(t, utts, T, true, t->xbuf.p, st));
  VCMI_TRY(traj_em_estep(t, du, 1, (int)T, T, true, st));
  int n = 0;
  VCMI_TRY(traj_em_scan(t, du, 1, T, T, st, &n));
  VCMI_TRY(traj_em_blend(t, pad != 0, n, st));
  VCMI_HIP(hipStreamSynchronize(st));
  VCMI_HIP(hipMemcpy(gamma, t->em_gamma.p, sizeof(double) * (size_t)T * M, hipMemcpyDeviceToHost));
  VCMI_HIP(hipMemcpy(lse, t->em_lse.p, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost));
  VCMI_HIP(hipMemcpy(flag, t->em_pure.p, sizeof(int32_t) * (size_t)T, hipMemcpyDeviceToHost));
  VCMI_HIP(hipMemcpy(gbar, t->gbuf.p, sizeof(double) * nx, hipMemcpyDeviceToHost));
  VCMI_HIP(hipMemcpy(mh, t->em_mh.p, sizeof(int64_t) * (size_t)T, hipMemcpyDeviceToHost));
  if (n > 0)
    VCMI_HIP(hipMemcpy(table, t->em_table.p + (size_t)M * (size_t)E, sizeof(double) * (size_t)n * (size_t)E, hipMemcpyDeviceToHost));
  *count = n;
  return VCMI_OK;
}

extern "C" int vcmi_traj_em_history(const vcmi_traj *t, double *L, int cap) {
  if (!t || (cap > 0 && !L) || cap < 0) return fail(VCMI_ERR_ARG, "vcmi_traj_em_history: bad argument");
  for (int k = 0; k < cap; ++k) L[k] = k < (int)t->em_hist.size() ? t->em_hist[(size_t)k] : NAN;
  return VCMI_OK;
}

extern "C" int vcmi_traj_cond_loglik_dev(vcmi_traj *t, const double *dX, const double *dY, int64_t T, double *dL, void *stream) {
  if (!t || !dL) return fail(VCMI_ERR_ARG, "vcmi_traj_cond_loglik_dev: NULL argument");
  if (T < 0 || T > INT32_MAX || (T > 0 && (!dX || !dY))) return fail(VCMI_ERR_ARG, "vcmi_traj_cond_loglik_dev: bad argument");
  if (t->b)      // (the E-step evaluates the dense model: not for a handle without one)
    return fail(VCMI_ERR_ARG, "vcmi_traj_cond_loglik: the converter was made from a cross-diagonal model (vcmi_traj_create_bdiag)");
  if (!t->em_pd) return fail(VCMI_ERR_NOT_PD, "vcmi_traj_cond_loglik: (Q_m + Q_m')/2 of some mixture is not positive definite");
  hipStream_t st = as_stream(stream);
  if (T == 0) {
    VCMI_HIP(hipMemsetAsync(dL, 0, sizeof(double), st));
    return VCMI_OK;
  }
  std::vector<TrajUtt> utts(1, TrajUtt{dX, const_cast<double *>(dY), 0, (int32_t)T, 0});
  VCMI_TRY(t->uttbuf.reserve(sizeof(TrajUtt)));
  VCMI_HIP(hipStreamSynchronize(st));       // (the descriptor buffer is shared with the conversion calls)
  VCMI_TRY(upload_now(t->uttbuf.p, utts.data(), sizeof(TrajUtt)));
  const TrajUtt *du = reinterpret_cast<const TrajUtt *>(t->uttbuf.p);
  VCMI_TRY(t->gbuf.reserve((size_t)T * t->D2));
  VCMI_TRY(traj_em_prior(t, utts, T, true, dX, st));
  VCMI_TRY(traj_em_estep(t, du, 1, (int)T, T, false, st));
  hipLaunchKernelGGL(traj_em_sum_kernel, dim3(1), dim3(256), 0, st, du, t->em_lse.p, dL);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

extern "C" int vcmi_traj_cond_loglik(vcmi_traj *t, const double *X, const double *Y, int64_t T, double *L) {
  if (!t || !L) return fail(VCMI_ERR_ARG, "vcmi_traj_cond_loglik: NULL argument");
  if (T < 0 || T > INT32_MAX || (T > 0 && (!X || !Y))) return fail(VCMI_ERR_ARG, "vcmi_traj_cond_loglik: bad argument");
  *L = 0.0;
  if (t->b)
    return fail(VCMI_ERR_ARG, "vcmi_traj_cond_loglik: the converter was made from a cross-diagonal model (vcmi_traj_create_bdiag)");
  if (T == 0) return VCMI_OK;
  VCMI_TRY(t->xbuf.reserve((size_t)T * t->D2));
  VCMI_TRY(t->ybuf.reserve((size_t)T * t->D + 1));
  VCMI_TRY(upload_now(t->xbuf.p, X, sizeof(double) * T * t->D2));
  VCMI_TRY(upload_now(t->ybuf.p, Y, sizeof(double) * T * t->D));
  double *dL = t->ybuf.p + (size_t)T * t->D;
  VCMI_TRY(vcmi_traj_cond_loglik_dev(t, t->xbuf.p, t->ybuf.p, T, dL, nullptr));
  VCMI_HIP(hipStreamSynchronize(nullptr));
  VCMI_HIP(hipMemcpy(L, dL, sizeof(double), hipMemcpyDeviceToHost));
  traj_em_release(t);
  return VCMI_OK;
}
