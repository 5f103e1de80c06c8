// traj_solve.hip -- the three banded Cholesky solvers of the trajectory normal equations (the math: header of traj.hip), their
// pad / unpad kernels, and the one dispatch behind traj_run and the EM loop (traj_internal.hpp: traj_solve_plan / _launch).
#include "traj_internal.hpp"
#include "traj_prepare.hpp"
#include "traj_band_plan.hpp"
#include "traj_blk_prof.hpp"
#include "hostpipe.hpp"
#include "lds_dma.hpp"

#include <algorithm>

namespace vcmi {

// ------------------------------------------------------------------------------------------------
// banded Cholesky solve, one workgroup (256 threads) per utterance
// ------------------------------------------------------------------------------------------------
// back substitution  L' y = z  from the panels in the HBM workspace (shared by both solve kernels).
// Panels are double-buffered in LDS (`buf`, 2 x PAN doubles): panel t-1 is fetched (coalesced, through registers)
// while step t computes.  The sequential part -- the D-step triangular solve -- runs in one wave with the needed
// row entries and reciprocal diagonal preloaded, so its chain is one shuffle + one FMA per step.
template <int NPRE>
__device__ void traj_backsub(const double *__restrict__ ws, size_t PAN, int D, int T, double *buf, double *yring, double *wv,
                             double *rdiag, double *__restrict__ Y) {
  const int tid = threadIdx.x, W3 = 3 * D;
#ifdef TRAJ_NO_BACKSUB
  return;
#endif
  for (int i = tid; i < 2 * D; i += 256) yring[i] = 0.0;
  {
    const double *pan = ws + (size_t)(T - 1) * PAN;
    for (size_t e = tid; e < PAN; e += 256) buf[((T - 1) & 1) * PAN + e] = pan[e];
  }
  __syncthreads();
  for (int t = T - 1; t >= 0; --t) {
    const double *pb = buf + (size_t)(t & 1) * PAN;
    double *pn = buf + (size_t)((t + 1) & 1) * PAN;       // receives panel t-1
    double pre[NPRE];
    if (t > 0) {
      const double *pan = ws + (size_t)(t - 1) * PAN;
#pragma unroll
      for (int k = 0; k < NPRE; ++k) {
        const size_t e = tid + (size_t)k * 256;
        pre[k] = (e < PAN) ? pan[e] : 0.0;
      }
    }
    double *y1 = yring + ((t + 1) & 1) * D, *y2 = yring + (t & 1) * D;   // y_{t+1}, y_{t+2}
    // w = z - E' y1 - F' y2  (thread j owns column j; panel rows D..3D-1 hold E then F)
    if (tid < D) {
      double s = pb[(size_t)W3 * D + tid];
      for (int i = 0; i < D; ++i) s = fma(-pb[(size_t)(D + i) * D + tid], y1[i], s);
      for (int i = 0; i < D; ++i) s = fma(-pb[(size_t)(2 * D + i) * D + tid], y2[i], s);
      wv[tid] = s;
    } else if (tid >= 64 && tid < 64 + D) {
      rdiag[tid - 64] = 1.0 / pb[(size_t)(tid - 64) * D + (tid - 64)];
    }
    __syncthreads();
    // Dg' y = w : sequential in k, one wave
    if (tid < 64) {
      double w = (tid < D) ? wv[tid] : 0.0;
      const double rd = (tid < D) ? rdiag[tid] : 0.0;
      for (int k = D - 1; k >= 0; --k) {
        const double lk = (tid < k) ? pb[(size_t)k * D + tid] : 0.0;   // independent of the chain: issued ahead
        const double yk = __shfl(w * rd, k);
        w = (tid == k) ? yk : fma(-lk, yk, w);
      }
      if (tid < D) {
        y2[tid] = w;                       // becomes y_t; the slot of y_{t+2} is free now
        Y[(size_t)t * D + tid] = w;        // reshape(y, D, T), src/trajectory_gmmmap.jl:109
      }
    }
    if (t > 0) {
#pragma unroll
      for (int k = 0; k < NPRE; ++k) {
        const size_t e = tid + (size_t)k * 256;
        if (e < PAN) pn[e] = pre[k];
      }
    }
    __syncthreads();
  }
}

// assemble global block row a of P (and r) into local block row la of the LDS window: blocks (a,a-2), (a,a-1), (a,a)
__device__ void traj_add_block_row(double *Wd, double *rr, int LD, int D, int a, int la, int T,
                                   const int64_t *__restrict__ mh, const double *__restrict__ g,
                                   const double *__restrict__ Qall) {
  const int tid = threadIdx.x, D2 = 2 * D;
  const double *Qa = Qall + (size_t)(mh[a] - 1) * D2 * D2;
  const double *Qm = (a >= 1) ? Qall + (size_t)(mh[a - 1] - 1) * D2 * D2 : nullptr;
  const double *Qp = (a + 1 < T) ? Qall + (size_t)(mh[a + 1] - 1) * D2 * D2 : nullptr;
  int i = tid / D, j = tid - i * D;                      // one division per call, then incremental
  const int di = 256 / D, dj = 256 - di * D;
  for (int e = tid; e < D * D; e += 256) {
    double *row = Wd + (size_t)(la * D + i) * LD;
    double v = Qa[(size_t)i * D2 + j];                                        // Qss(a)
    if (Qm) v += 0.25 * Qm[(size_t)(D + i) * D2 + (D + j)];                   // + Qdd(a-1)/4
    if (Qp) v += 0.25 * Qp[(size_t)(D + i) * D2 + (D + j)];                   // + Qdd(a+1)/4
    row[la * D + j] = v;
    if (la >= 1 && a >= 1)
      row[(la - 1) * D + j] = 0.5 * Qm[(size_t)(D + i) * D2 + j] - 0.5 * Qa[(size_t)i * D2 + (D + j)];   // Qds(a-1)/2 - Qsd(a)/2
    if (la >= 2 && a >= 2)
      row[(la - 2) * D + j] = -0.25 * Qm[(size_t)(D + i) * D2 + (D + j)];     // -Qdd(a-1)/4
    i += di;
    j += dj;
    if (j >= D) { j -= D; ++i; }
  }
  for (int k = tid; k < D; k += 256) {
    double v = g[(size_t)a * D2 + k];
    if (a >= 1) v += 0.5 * g[(size_t)(a - 1) * D2 + D + k];
    if (a + 1 < T) v -= 0.5 * g[(size_t)(a + 1) * D2 + D + k];
    rr[la * D + k] = v;
  }
}

// LDS window: rows/cols 0..3D-1 = global rows t*D .. t*D+3D-1 of the band (row stride LD); after block column t is
// finished the lower-right 2D x 2D part is shifted up-left by D (through registers) and block row t+3 is assembled
// into the freed rows.  No index arithmetic beyond adds in the hot loops.
static constexpr int kBackPre = (139 * 46 + 255) / 256;   // panel doubles per thread for the largest supported D
static constexpr int kShiftRegs = 36;   // ceil(4*46^2 / 256) doubles per thread for the window shift

__global__ void __launch_bounds__(256)
traj_solve_kernel(const TrajUtt *__restrict__ utts, int n, int D, const double *__restrict__ Qall,
                  const int64_t *__restrict__ mhat_all, const double *__restrict__ g_all, double *__restrict__ ws_all,
                  int64_t ws_stride, int *__restrict__ status) {
  const int D2 = 2 * D, W3 = 3 * D, LD = W3 + 1;
  extern __shared__ double sm[];
  double *Wd = sm;                       // [W3][LD]
  double *rr = Wd + (size_t)W3 * LD;     // [W3] right-hand side riding along as an extra row
  double *lcol = rr + W3;                // [W3] scaled pivot column of the current elimination step
  double *yring = lcol + W3;             // [2][D]  y_{t+1}, y_{t+2} during back-substitution
  double *wv = yring + 2 * D;            // [D]
  __shared__ int bad;
  __shared__ double zc_s;
  const int tid = threadIdx.x;
  const int ti = tid >> 4, tj = tid & 15;
  const size_t PAN = (size_t)(W3 + 1) * D;   // panel: rows 0..3D-1 of L[:, block t] (relative to t) + z row

  for (int u = blockIdx.x; u < n; u += gridDim.x) {
    const TrajUtt U = utts[u];
    const int T = U.T;
    if (T == 0) continue;
    const int64_t *mh = mhat_all + U.frame0;
    const double *g = g_all + U.frame0 * D2;
    double *ws = ws_all + (size_t)blockIdx.x * ws_stride;
    if (tid == 0) bad = 0;

    auto add_block_row = [&](int a, int la) { traj_add_block_row(Wd, rr, LD, D, a, la, T, mh, g, Qall); };

    for (int a = 0; a < 3 && a < T; ++a) add_block_row(a, a);
    __syncthreads();

    // ---------------- factorisation + forward substitution ----------------
    for (int t = 0; t < T; ++t) {
      const int nb = (T - t < 3) ? T - t : 3;      // block rows alive in the window
      const int nrows = nb * D;
      for (int c = 0; c < D; ++c) {
        // (a) pivot and scaled column into lcol (the window column itself is left untouched until (b))
        const double piv = Wd[(size_t)c * LD + c];
        if (!(piv > 0.0) && tid == 0) bad = 1;
        const double dinv = traj_rsqrt(piv);
        for (int lr = c + tid; lr < nrows; lr += 256) lcol[lr] = (lr == c) ? piv * dinv : Wd[(size_t)lr * LD + c] * dinv;
        if (tid == 255) zc_s = rr[c] * dinv;
        __syncthreads();
        // (b) rank-1 update of the trailing lower triangle and of the rhs; the finished column goes back to the window
        const int rem = nrows - c - 1;
        for (int a = ti; a < rem; a += 16) {
          const int ri = c + 1 + a;
          const double lic = lcol[ri];
          double *row = Wd + (size_t)ri * LD + c + 1;
          for (int b = tj; b <= a; b += 16) row[b] = fma(-lic, lcol[c + 1 + b], row[b]);
        }
        const double zc = zc_s;
        for (int lr = c + tid; lr < nrows; lr += 256) {
          Wd[(size_t)lr * LD + c] = lcol[lr];
          if (lr > c) rr[lr] = fma(-zc, lcol[lr], rr[lr]);
          else rr[lr] = zc;
        }
        __syncthreads();
      }
      // stream the finished panel: rows 0..3D-1 (zero beyond nrows), columns of block t; then the z row
      double *pan = ws + (size_t)t * PAN;
      {
        int lr = tid / D, cc = tid - lr * D;
        const int dl = 256 / D, dc = 256 - dl * D;
        for (int e = tid; e < W3 * D; e += 256) {
          pan[e] = (lr < nrows) ? Wd[(size_t)lr * LD + cc] : 0.0;
          lr += dl;
          cc += dc;
          if (cc >= D) { cc -= D; ++lr; }
        }
      }
      for (int cc = tid; cc < D; cc += 256) pan[(size_t)W3 * D + cc] = rr[cc];
      // shift the window up-left by D (through registers), then assemble block row t+3
      double sh[kShiftRegs];
      double rsh = 0.0;
      {
        int i = tid / D2, j = tid - i * D2;
        const int di = 256 / D2, dj = 256 - di * D2;
#pragma unroll
        for (int k = 0; k < kShiftRegs; ++k) {
          sh[k] = (i < D2) ? Wd[(size_t)(i + D) * LD + (j + D)] : 0.0;
          i += di;
          j += dj;
          if (j >= D2) { j -= D2; ++i; }
        }
        if (tid < D2) rsh = rr[tid + D];
      }
      __syncthreads();
      {
        int i = tid / D2, j = tid - i * D2;
        const int di = 256 / D2, dj = 256 - di * D2;
#pragma unroll
        for (int k = 0; k < kShiftRegs; ++k) {
          if (i < D2) Wd[(size_t)i * LD + j] = sh[k];
          i += di;
          j += dj;
          if (j >= D2) { j -= D2; ++i; }
        }
        if (tid < D2) rr[tid] = rsh;
      }
      if (t + 3 < T) add_block_row(t + 3, 2);
      __syncthreads();
    }

    traj_backsub<kBackPre>(ws, PAN, D, T, Wd, yring, wv, lcol, U.Y);
    if (tid == 0 && bad) status[0] = 1;
    __syncthreads();
  }
}

#include "traj_solve_blk.hpp"

// g (frames x [gs (D); gd (D)]) -> gpad (frames x [gs (Dp); gd (Dp)]), zeros in the padding
__global__ void __launch_bounds__(256)
traj_pad_g_kernel(const double *__restrict__ g, int64_t nframes, int D, int Dp, double *__restrict__ gpad) {
  const int64_t n = nframes * 2 * Dp;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t f = e / (2 * Dp);
    const int c = (int)(e - f * 2 * Dp), half = c / Dp, d = c - half * Dp;
    gpad[e] = (d < D) ? g[f * 2 * D + half * D + d] : 0.0;
  }
}
// ypad (frames x Dp) -> the utterances' own (T, D) outputs
__global__ void __launch_bounds__(256)
traj_unpad_y_kernel(const TrajUtt *__restrict__ utts, const double *__restrict__ ypad, int D, int Dp) {
  const TrajUtt u = utts[blockIdx.x];
  const int64_t n = (int64_t)u.T * D;
  for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.y * 256) {
    const int64_t tt = e / D;
    u.Y[e] = ypad[(u.frame0 + tt) * Dp + (e - tt * D)];
  }
}

// ------------------------------------------------------------------------------------------------
// Any static dimension (D >= 47: the reference has no limit, src/trajectory_gmmmap.jl:65-110): the algorithm of
// traj_solve_kernel with its 3D x 3D window, right-hand side, pivot column and the vectors of the back substitution in HBM
// (a per-workgroup scratch, L2-resident) instead of LDS -- a fallback for completeness, not a fast path: every
// __syncthreads also orders the workgroup's global accesses.  Window shift through a second buffer; the triangular solve of
// the back substitution column by column across the workgroup.
// ------------------------------------------------------------------------------------------------
static size_t traj_big_win_doubles(int D) {
  const size_t W3 = 3 * (size_t)D, D2 = 2 * (size_t)D;
  return W3 * (W3 + 1) + 2 * W3 + 2 * D + 2 * D + D2 * D2 + D2 + 64;
}

// PK = true (47 <= D <= 64): the window's LOWER TRIANGLE in packed storage, (i, j <= i) at i (i + 1) / 2 + j, fits LDS
// (148 KB at D = 64) together with the small vectors; only the shift buffer and the panels stay in HBM.  PK = false: everything
// in the per-workgroup HBM scratch.
static size_t traj_big_lds_bytes(int D) {
  const size_t W3 = 3 * (size_t)D;
  return (W3 * (W3 + 1) / 2 + 2 * W3 + 2 * D + 2 * D + 8) * sizeof(double);
}

template <bool PK>
__global__ void __launch_bounds__(256)
traj_solve_big_kernel(const TrajUtt *__restrict__ utts, int n, int D, const double *__restrict__ Qall,
                      const int64_t *__restrict__ mhat_all, const double *__restrict__ g_all, double *__restrict__ ws_all,
                      int64_t ws_stride, int *__restrict__ status, double *__restrict__ gwin_all, int64_t gwin_stride) {
  const int D2 = 2 * D, W3 = 3 * D, LD = W3 + 1;
  extern __shared__ double sm_big[];
  double *gw = gwin_all + (size_t)blockIdx.x * gwin_stride;
  double *Wd = PK ? sm_big : gw;                                   // the window: packed lower triangle (LDS) or [W3][LD] (HBM)
  double *vec = PK ? sm_big + (size_t)W3 * (W3 + 1) / 2 : gw + (size_t)W3 * LD;
  double *rr = vec;                      // [W3]
  double *lcol = rr + W3;                // [W3]
  double *yring = lcol + W3;             // [2][D]
  double *wv = yring + 2 * D;            // [D]
  double *rdiag = wv + D;                // [D]
  double *tmp = PK ? gw : rdiag + D;     // [D2][D2] + [D2] in HBM: the shifted part of the window on its way up-left
  auto W = [&](int i, int j) -> double & { return PK ? Wd[(size_t)i * (i + 1) / 2 + j] : Wd[(size_t)i * LD + j]; };
  __shared__ int bad;
  __shared__ double zc_s;
  const int tid = threadIdx.x;
  const int ti = tid >> 4, tj = tid & 15;
  const size_t PAN = (size_t)(W3 + 1) * D;

  for (int u = blockIdx.x; u < n; u += gridDim.x) {
    const TrajUtt U = utts[u];
    const int T = U.T;
    if (T == 0) continue;
    const int64_t *mh = mhat_all + U.frame0;
    const double *g = g_all + U.frame0 * D2;
    double *ws = ws_all + (size_t)blockIdx.x * ws_stride;
    if (tid == 0) bad = 0;
    // block row a of P (blocks (a,a-2), (a,a-1), (a,a): traj_add_block_row's terms) into window block row la; lower triangle only
    auto add_block_row = [&](int a, int la) {
      const double *Qa = Qall + (size_t)(mh[a] - 1) * D2 * D2;
      const double *Qm = (a >= 1) ? Qall + (size_t)(mh[a - 1] - 1) * D2 * D2 : nullptr;
      const double *Qp = (a + 1 < T) ? Qall + (size_t)(mh[a + 1] - 1) * D2 * D2 : nullptr;
      for (int e = tid; e < D * D; e += 256) {
        const int i = e / D, j = e - i * D;
        if (j <= i) {
          double v = Qa[(size_t)i * D2 + j];
          if (Qm) v += 0.25 * Qm[(size_t)(D + i) * D2 + (D + j)];
          if (Qp) v += 0.25 * Qp[(size_t)(D + i) * D2 + (D + j)];
          W(la * D + i, la * D + j) = v;
        }
        if (la >= 1 && a >= 1) W(la * D + i, (la - 1) * D + j) = 0.5 * Qm[(size_t)(D + i) * D2 + j] - 0.5 * Qa[(size_t)i * D2 + (D + j)];
        if (la >= 2 && a >= 2) W(la * D + i, (la - 2) * D + j) = -0.25 * Qm[(size_t)(D + i) * D2 + (D + j)];
      }
      for (int k = tid; k < D; k += 256) {
        double v = g[(size_t)a * D2 + k];
        if (a >= 1) v += 0.5 * g[(size_t)(a - 1) * D2 + D + k];
        if (a + 1 < T) v -= 0.5 * g[(size_t)(a + 1) * D2 + D + k];
        rr[la * D + k] = v;
      }
    };
    for (int a = 0; a < 3 && a < T; ++a) add_block_row(a, a);
    __syncthreads();
    for (int t = 0; t < T; ++t) {
      const int nb = (T - t < 3) ? T - t : 3;
      const int nrows = nb * D;
      for (int c = 0; c < D; ++c) {
        const double piv = W(c, c);
        if (!(piv > 0.0) && tid == 0) bad = 1;
        const double dinv = traj_rsqrt(piv);
        for (int lr = c + tid; lr < nrows; lr += 256) lcol[lr] = (lr == c) ? piv * dinv : W(lr, c) * dinv;
        if (tid == 255) zc_s = rr[c] * dinv;
        __syncthreads();
        const int rem = nrows - c - 1;
        for (int a = ti; a < rem; a += 16) {
          const int ri = c + 1 + a;
          const double lic = lcol[ri];
          double *row = &W(ri, c + 1);
          for (int b = tj; b <= a; b += 16) row[b] = fma(-lic, lcol[c + 1 + b], row[b]);
        }
        const double zc = zc_s;
        for (int lr = c + tid; lr < nrows; lr += 256) {
          W(lr, c) = lcol[lr];
          if (lr > c) rr[lr] = fma(-zc, lcol[lr], rr[lr]);
          else rr[lr] = zc;
        }
        __syncthreads();
      }
      double *pan = ws + (size_t)t * PAN;
      for (int e = tid; e < W3 * D; e += 256) {
        const int lr = e / D, cc = e - lr * D;
        pan[e] = (lr < nrows && cc <= lr) ? W(lr, cc) : 0.0;
      }
      for (int cc = tid; cc < D; cc += 256) pan[(size_t)W3 * D + cc] = rr[cc];
      // the lower-right 2D x 2D part (its lower triangle) moves up-left by D
      for (int e = tid; e < D2 * D2; e += 256) {
        const int i = e / D2, j = e - i * D2;
        if (j <= i) tmp[e] = W(i + D, j + D);
      }
      for (int k = tid; k < D2; k += 256) tmp[(size_t)D2 * D2 + k] = rr[k + D];
      __syncthreads();
      for (int e = tid; e < D2 * D2; e += 256) {
        const int i = e / D2, j = e - i * D2;
        if (j <= i) W(i, j) = tmp[e];
      }
      for (int k = tid; k < D2; k += 256) rr[k] = tmp[(size_t)D2 * D2 + k];
      __syncthreads();
      if (t + 3 < T) add_block_row(t + 3, 2);
      __syncthreads();
    }
    // ---------------- back substitution: y_t = Dg'^-1 (z - E' y_{t+1} - F' y_{t+2}) from the panels ----------------
    for (int i = tid; i < 2 * D; i += 256) yring[i] = 0.0;
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
      const double *pb = ws + (size_t)t * PAN;
      if (PK) {
        // the panel into the (now free) window area first, by all threads: the sums and the column-by-column solve below then
        // read LDS instead of walking HBM with one dependent load after the other (PAN <= W3 (W3 + 1) / 2 for every D)
        for (size_t e = tid; e < PAN; e += 256) sm_big[e] = pb[e];
        __syncthreads();
        pb = sm_big;
      }
      double *y1 = yring + ((t + 1) & 1) * D, *y2 = yring + (t & 1) * D;
      for (int j = tid; j < D; j += 256) {
        double sacc = pb[(size_t)W3 * D + j];
        for (int i = 0; i < D; ++i) sacc = fma(-pb[(size_t)(D + i) * D + j], y1[i], sacc);
        for (int i = 0; i < D; ++i) sacc = fma(-pb[(size_t)(2 * D + i) * D + j], y2[i], sacc);
        wv[j] = sacc;
        rdiag[j] = 1.0 / pb[(size_t)j * D + j];
      }
      for (int k = D - 1; k >= 0; --k) {
        __syncthreads();
        const double yk = wv[k] * rdiag[k];
        for (int j = tid; j < k; j += 256) wv[j] = fma(-pb[(size_t)k * D + j], yk, wv[j]);
        if (tid == 0) {
          lcol[k] = yk;                      // (lcol is free during the back substitution)
          U.Y[(size_t)t * D + k] = yk;
        }
      }
      __syncthreads();
      for (int j = tid; j < D; j += 256) y2[j] = lcol[j];
      __syncthreads();
    }
    if (tid == 0 && bad) status[0] = 1;
    __syncthreads();
  }
}

static size_t solve_lds_bytes(int D) {
  const size_t W3 = 3 * (size_t)D;
  const size_t NK = (W3 + 15) / 16;
  return (W3 * (W3 + 1) + 2 * W3 + 2 * (NK * 16 + 2) + 2 * D + D) * sizeof(double);   // covers both solve kernels
}

// ---- host side: one plan per call, one launch function ------------------------------------------
bool traj_solve_is_big(int D) { return solve_lds_bytes(D) > 160 * 1024 - 64; }

// The blocked solver of the (sorted) utterances [b0, b0 + nb) in static dimension DV.  With occ (the plan's call) nothing is
// launched: the kernels get their LDS sizes and *occ the workgroups a CU holds at once (two where LDS and registers allow).
template <int DV>
static int launch_blk(vcmi_traj *t, const TrajSolvePlan &p, int *occ, const double *Qs, const int64_t *mh, int b0, int nb, hipStream_t st) {
  auto kern = traj_solve_blk_kernel<DV>;
  auto kb = traj_backsub_blk_kernel<DV>;
  const size_t shb = BlkCfg<DV>::lds_doubles * sizeof(double), shs = blk_backsub_lds_bytes<DV>();
  if (occ) {
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shb));
    if (debug_flag(kDbgTrajOneWgPerCu) ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, kern, blk_threads<DV>(), shb) != hipSuccess || *occ < 1)
      *occ = 1;
    if (!blk_fused_backsub<DV>())
      VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kb), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shs));
    return VCMI_OK;
  }
  const int grid_blk = (int)std::min<int64_t>(nb, (int64_t)p.cus * p.occ);
  if (blk_fused_backsub<DV>()) {
    hipLaunchKernelGGL(kern, dim3(grid_blk), dim3(blk_threads<DV>()), shb, st, p.dus + b0, nb, Qs, mh, p.gs, t->ws.p, p.ws_stride_s,
                       t->status.p);
    return VCMI_OK;
  }
  // eight waves: factorisation and back substitution are two kernels, per batch of grid_blk utterances
  for (int c0 = 0; c0 < nb; c0 += grid_blk) {
    const int nc = std::min(grid_blk, nb - c0);
    hipLaunchKernelGGL(kern, dim3(nc), dim3(blk_threads<DV>()), shb, st, p.dus + b0 + c0, nc, Qs, mh, p.gs, t->ws.p, p.ws_stride_s,
                       t->status.p);
    hipLaunchKernelGGL(kb, dim3(nc), dim3(BacksubCfg<DV>::THREADS), shs, st, p.dus + b0 + c0, nc, t->ws.p, p.ws_stride_s);
  }
  return VCMI_OK;
}
static int dispatch_blk(vcmi_traj *t, const TrajSolvePlan &p, int *occ, const double *Qs, const int64_t *mh, int b0, int nb, hipStream_t st) {
  switch (p.Ds) {
#define VCMI_TRAJ_BLK_CASE_(DV) \
  case DV: return launch_blk<DV>(t, p, occ, Qs, mh, b0, nb, st);
    VCMI_TRAJ_BLK_DIMS(VCMI_TRAJ_BLK_CASE_)
#undef VCMI_TRAJ_BLK_CASE_
    default: return VCMI_OK;
  }
}

int traj_solve_plan(vcmi_traj *t, const std::vector<TrajUtt> &utts, int64_t nframes, int Tmax, bool with_gv, TrajSolvePlan *plan) {
  TrajSolvePlan &p = *plan;
  p = TrajSolvePlan();
  const int D = t->D, n = (int)utts.size();
  p.n = n;
  p.Tmax = Tmax;
  p.nframes = nframes;
  int dev = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&p.cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (t->precision == VCMI_TRAJ_PRECISION_DIAG) {   // the band family: (nframes,D) arrays indexed by frame0; nothing else
    p.Ds = D;
    p.du = p.dus = reinterpret_cast<const TrajUtt *>(t->uttbuf.p);
    p.gs = t->gbuf.p;
    p.grid = std::min(n, p.cus);            // workgroups of the GV ascent (traj_gvd_kernel, traj_gvp_kernel)
    // the whole reserve, not a stride: traj_band_gv_launch checks it
    p.ws_stride = band_ws_doubles(t->windows, nframes, D, with_gv);
    return t->ws.reserve((size_t)p.ws_stride);
  }
  p.grid = std::min(n, p.cus);
  p.ws_stride = (int64_t)Tmax * (3 * D + 1) * D;
  if (with_gv) p.ws_stride = std::max<int64_t>(p.ws_stride, (int64_t)Tmax * 3 * D + (17 * (int64_t)Tmax + 1) / 2 + 16);   // V, r, perm
  // the dimension the blocked solver runs in, and its operands: the utterances' own, or the padded copies
  p.padded = t->Dpad && !debug_flag(kDbgTrajGeneric);
  p.Ds = p.padded ? t->Dpad : D;
  p.blk = !debug_flag(kDbgTrajGeneric) && traj_blk_has(p.Ds);
  p.du = p.dus = reinterpret_cast<const TrajUtt *>(t->uttbuf.p);
  p.gs = t->gbuf.p;
  p.ws_stride_s = p.ws_stride;
  if (p.padded) {
    const int Dp = t->Dpad;
    VCMI_TRY(t->gpad.reserve((size_t)nframes * 2 * Dp));
    VCMI_TRY(t->ypad.reserve((size_t)nframes * Dp));
    VCMI_TRY(t->uttpad.reserve(sizeof(TrajUtt) * n));
    std::vector<TrajUtt> up(utts);
    for (auto &u : up) u.Y = t->ypad.p + (size_t)u.frame0 * Dp;
    VCMI_TRY(upload_now(t->uttpad.p, up.data(), sizeof(TrajUtt) * n));
    p.ws_stride_s = (int64_t)Tmax * (3 * Dp + 1) * Dp;
    p.gs = t->gpad.p;
    p.dus = reinterpret_cast<const TrajUtt *>(t->uttpad.p);
  }
  if (p.blk) VCMI_TRY(dispatch_blk(t, p, &p.occ, nullptr, nullptr, 0, 0, nullptr));
  // one workspace per workgroup of the widest launch, + slack: the blocked back substitution reads whole kilobytes
  const int64_t wgs = p.blk ? std::max<int64_t>(p.grid, std::min<int64_t>(n, (int64_t)p.cus * p.occ)) : p.grid;
  VCMI_TRY(t->ws.reserve((size_t)wgs * std::max(p.ws_stride, p.ws_stride_s) + 256));
  if (!p.blk && t->big) VCMI_TRY(t->gwin.reserve((size_t)p.grid * traj_big_win_doubles(D)));
  return VCMI_OK;
}

int traj_solve_launch(vcmi_traj *t, const TrajSolvePlan &p, const double *Qs, const int64_t *mh, int b0, int nb, hipStream_t st) {
  const int D = t->D, grid_s = std::min(nb, p.cus);
  if (p.padded) {   // gbuf -> gpad
    hipLaunchKernelGGL(traj_pad_g_kernel, dim3((unsigned)std::min<int64_t>((p.nframes * 2 * t->Dpad + 255) / 256, 4096)), dim3(256), 0, st,
                       t->gbuf.p, p.nframes, D, t->Dpad, t->gpad.p);
    VCMI_HIP(hipGetLastError());
  }
  if (p.blk) {
    VCMI_TRY(dispatch_blk(t, p, nullptr, Qs, mh, b0, nb, st));
    if (t->Dpad) {
      hipLaunchKernelGGL(traj_unpad_y_kernel, dim3(nb, 8), dim3(256), 0, st, p.du + b0, t->ypad.p, D, t->Dpad);
      VCMI_HIP(hipGetLastError());
    }
  } else if (t->big) {
    const size_t lds_pk = traj_big_lds_bytes(D);
    const bool pk = lds_pk <= 160 * 1024 - 256;       // D <= 64: the window's lower triangle in LDS
    auto kern = pk ? traj_solve_big_kernel<true> : traj_solve_big_kernel<false>;
    if (pk) VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_pk));
    hipLaunchKernelGGL(kern, dim3(grid_s), dim3(256), pk ? lds_pk : 0, st, p.du + b0, nb, D, Qs, mh, t->gbuf.p, t->ws.p, p.ws_stride,
                       t->status.p, t->gwin.p, (int64_t)traj_big_win_doubles(D));
  } else {
    const size_t shmem = solve_lds_bytes(D);
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(traj_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)shmem));
    hipLaunchKernelGGL(traj_solve_kernel, dim3(grid_s), dim3(256), shmem, st, p.du + b0, nb, D, Qs, mh, t->gbuf.p, t->ws.p,
                       p.ws_stride, t->status.p);
  }
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

#ifdef TRAJ_BLK_PROF
void traj_solve_prof_dump(hipStream_t st) {
  long long h[32];
  blk_prof_fetch(h, st);
  fprintf(stderr, "blk_prof cycles: phase1 %lld trsm %lld update %lld backsub %lld | pivot S done at %lld, pivot U at %lld, deferred: S21/S22 at %lld, panel+assembly at %lld\n",
          h[0], h[1], h[2], h[5], h[3], h[4], h[6], h[7]);
  fprintf(stderr, "   deferred wave 2: L20 done %lld, S21/S22 done %lld, loads issued %lld, panel stored %lld, combined %lld | wave 0 jobs done %lld, wave 1 jobs done %lld | wave 3: S21/S22 done %lld, combined %lld\n", h[8],
          h[6], h[10], h[11], h[7], h[9], h[12], h[14], h[13]);
  fprintf(stderr, "   deferred waves 2..7: S21/S22 jobs done %lld %lld %lld %lld %lld %lld | at the barrier %lld %lld %lld %lld %lld %lld\n", h[26], h[27], h[28],
          h[29], h[30], h[31], h[18], h[19], h[20], h[21], h[22], h[23]);
}
#endif

}  // namespace vcmi
