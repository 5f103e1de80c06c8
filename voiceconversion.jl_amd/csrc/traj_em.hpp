// traj_em.hpp -- EM re-estimation of the trajectory over ALL mixtures (Toda, Black, Tokuda 2007, eqs. 30-36) in place of the
// suboptimum mixture sequence of src/trajectory_gmmmap.jl:81-82 (their eq. 37).  Included by traj.hip (shares its statics).
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
#pragma once

static constexpr int kEmNB = 4;              // 16-frame tiles per workgroup of the MFMA kernels
static constexpr int kEmF = 16 * kEmNB;      // ... frames
static constexpr double kEmLog2Pi = 1.8378770664093454835606594728112;

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

// l_{m,.} of one frame (written by the calling thread itself) -> gamma, lse, flag.  A frame is PURE when 1 - max gamma < 2^-53:
// it takes that mixture alone (gamma written one-hot, flag = its index); otherwise MIXED (flag -1).
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
// reads (Q, or Qpad: sum gamma = 1 keeps the padding's unit diagonal).  A operand: gamma of the tile's 16 frames, four
// mixtures per k-step; B operand: 16 consecutive elements of those four matrices.  grid (mixed tiles, element chunks), a wave
// per 16-element column block.  2 M E flop, E doubles written per frame.
__global__ void __launch_bounds__(256)
traj_em_blend_kernel(const double *__restrict__ Qtab, int M, int64_t E, const double *__restrict__ gam_all,
                     const int *__restrict__ mix, int count, double *__restrict__ out) {
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
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t k = k0 + lgrp + 4 * r;
      if (k < count && el < E) out[(size_t)k * E + el] = acc[r];
    }
  }
}

