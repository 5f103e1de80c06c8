// traj_gv_band.hpp -- the frame of the global-variance ascents over diagonal conditional precisions, once, and the two stencils
// that run in it (traj_gv_band.hip makes traj_gvd_kernel and traj_gvp_kernel of them).  Device code.
//
// With D^-1 = diag(q) the likelihood gradient per static dimension is omega (r - P y) with the symmetric banded P and the r that
// the solver of the handle factorises (traj_gv_band_step.hpp states them by column, with W's boundaries).  The epoch
//   y <- y + alpha ( omega (r - P y) + coef (.) (y - mean) ),   coef = -2/T pv' (var_1(y) - mu_v),   omega = 1/(2T)
// is a JACOBI step: the neighbours of y_t are the previous epoch's, so y has two buffers that swap per epoch.
#pragma once
#include "traj_internal.hpp"
#include "traj_band_plan.hpp"
#include "traj_gv_band_step.hpp"
#include "traj_gv_moments.hpp"

namespace vcmi {

// an array of the ascent lives in LDS or in global memory, decided per instantiation: the accesses are ds_ / global_
// instructions, never flat ones
template <bool LDS>
struct BandPtr {
  typedef gdouble *type;
};
template <>
struct BandPtr<true> {
  typedef double *type;
};
// array K of the ascent in the order of traj_band_plan.hpp (0 and 1: the two y), with NRES of them in LDS: at arr in LDS, else
// at glob
template <int K, int NRES>
__device__ __forceinline__ typename BandPtr<(NRES > K)>::type band_sel(double *arr, int64_t lds_arr, gdouble *glob) {
  if constexpr (NRES > K) return arr + K * lds_arr;
  else return glob;
}

// ------------------------------------------------------------------------------------------------
// A stencil is what differs between the window counts.  It keeps its coefficient arrays (array 2 onwards, each in LDS or in the
// workspace: wsu is the utterance's part of array 1, `stride` doubles lie between arrays) and supplies
//   kArrays, kWindows (features per frame: kWindows * D), kBatch (frames a thread has in flight in the epoch), kPrologueUnroll;
//   coefficients(), store(): c and r of frame t from the dependent gathers q[mhat_{t-1}], q[mhat_t], q[mhat_{t+1}] and g;
//   load():     what an epoch reads for frame tc of T, every load unconditional on an address clamped into the utterance
//               (T >= 2): a coefficient below its first frame is stored as zero, what is loaded for a frame past the end gets
//               weight zero in the step;
//   step():     the new y_t.
// ------------------------------------------------------------------------------------------------
template <int NRES>
struct GvdStencil {      // two windows: (P y)_t = c0_t y_t + c2_t y_{t-2} + c2_{t+2} y_{t+2}, 7 loads per element
  static constexpr int kArrays = kGvdArrays, kWindows = 2, kBatch = 4, kPrologueUnroll = 4;
  const typename BandPtr<(NRES > 2)>::type C2;
  const typename BandPtr<(NRES > 3)>::type C0;
  const typename BandPtr<(NRES > 4)>::type R;
  struct Loaded {
    double yc, ym, yp, rr, a0, am, ap;
  };
  __device__ __forceinline__ GvdStencil(double *arr, int64_t lds_arr, gdouble *wsu, int64_t stride)
      : C2(band_sel<2, NRES>(arr, lds_arr, wsu + stride)), C0(band_sel<3, NRES>(arr, lds_arr, wsu + 2 * stride)),
        R(band_sel<4, NRES>(arr, lds_arr, wsu + 3 * stride)) {}
  __device__ __forceinline__ GvdCoef coefficients(int t, int T, int D, int d, const double *q, const int64_t *mh, const double *g) const {
    const int D2 = 2 * D;
    const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
    const int m0 = (int)mh[t] - 1, mm = (int)mh[tm] - 1, mp = (int)mh[tp] - 1;
    const double ps = q[(size_t)m0 * D2 + d], pdm = q[(size_t)mm * D2 + D + d], pdp = q[(size_t)mp * D2 + D + d];
    const double g0 = g[(size_t)t * D2 + d], g1 = g[(size_t)tm * D2 + D + d], g2 = g[(size_t)tp * D2 + D + d];
    return gvd_coefficients(ps, pdm, pdp, g0, g1, g2, t, T);
  }
  __device__ __forceinline__ void store(size_t e, const GvdCoef &c) const {
    R[e] = c.r;
    C0[e] = c.c0;
    C2[e] = c.c2;
  }
  template <typename YP>
  __device__ __forceinline__ Loaded load(YP src, int tc, int T, int D, int d) const {
    const int tm = tc >= 2 ? tc - 2 : tc, tp = tc + 2 < T ? tc + 2 : tc;
    const size_t ec = (size_t)tc * D + d, em = (size_t)tm * D + d, ep2 = (size_t)tp * D + d;
    Loaded l;
    l.yc = src[ec];
    l.ym = src[em];
    l.yp = src[ep2];
    l.rr = R[ec];
    l.a0 = C0[ec];
    l.am = C2[ec];
    l.ap = C2[ep2];
    return l;
  }
  static __device__ __forceinline__ double step(const Loaded &l, int t, int T, double omega, double cf, double mu, double alpha) {
    return gvd_epoch_step(l.yc, l.ym, l.yp, l.a0, l.am, l.ap, l.rr, t, T, omega, cf, mu, alpha);
  }
};

template <int NRES>
struct GvpStencil {      // three windows: c1_t y_{t-1} + c1_{t+1} y_{t+1} on top, 11 loads per element
  static constexpr int kArrays = kGvpArrays, kWindows = 3, kBatch = 4, kPrologueUnroll = 2;
  const typename BandPtr<(NRES > 2)>::type C1;
  const typename BandPtr<(NRES > 3)>::type C2;
  const typename BandPtr<(NRES > 4)>::type C0;
  const typename BandPtr<(NRES > 5)>::type R;
  struct Loaded {
    double y0, ym1, yp1, ym2, yp2, rr, a0, a1, a1n, a2, a2n;
  };
  __device__ __forceinline__ GvpStencil(double *arr, int64_t lds_arr, gdouble *wsu, int64_t stride)
      : C1(band_sel<2, NRES>(arr, lds_arr, wsu + stride)), C2(band_sel<3, NRES>(arr, lds_arr, wsu + 2 * stride)),
        C0(band_sel<4, NRES>(arr, lds_arr, wsu + 3 * stride)), R(band_sel<5, NRES>(arr, lds_arr, wsu + 4 * stride)) {}
  __device__ __forceinline__ GvpCoef coefficients(int t, int T, int D, int d, const double *q, const int64_t *mh, const double *g) const {
    const int D3 = 3 * D;
    const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
    const double *q0 = q + (size_t)((int)mh[t] - 1) * D3 + d, *qm = q + (size_t)((int)mh[tm] - 1) * D3 + d,
                 *qp = q + (size_t)((int)mh[tp] - 1) * D3 + d;
    const double *g0 = g + (size_t)t * D3 + d, *gm = g + (size_t)tm * D3 + d, *gp = g + (size_t)tp * D3 + d;
    const PentaRow cur{q0[0], q0[D], q0[2 * D], g0[0], g0[D], g0[2 * D]};
    const PentaRow prv{0.0, qm[D], qm[2 * D], 0.0, gm[D], gm[2 * D]};     // (the static parts of a neighbour are not read)
    const PentaRow nxt{0.0, qp[D], qp[2 * D], 0.0, gp[D], gp[2 * D]};
    return gvp_coefficients(prv, cur, nxt, t, T);
  }
  __device__ __forceinline__ void store(size_t e, const GvpCoef &c) const {
    C0[e] = c.c0;
    C1[e] = c.c1;
    C2[e] = c.c2;
    R[e] = c.r;
  }
  template <typename YP>
  __device__ __forceinline__ Loaded load(YP src, int tc, int T, int D, int d) const {
    const int t1m = tc >= 1 ? tc - 1 : tc, t1p = tc + 1 < T ? tc + 1 : tc;
    const int t2m = tc >= 2 ? tc - 2 : tc, t2p = tc + 2 < T ? tc + 2 : tc;
    const size_t ec = (size_t)tc * D + d, e1m = (size_t)t1m * D + d, e1p = (size_t)t1p * D + d, e2m = (size_t)t2m * D + d,
                 e2p = (size_t)t2p * D + d;
    Loaded l;
    l.y0 = src[ec];
    l.ym1 = src[e1m];
    l.yp1 = src[e1p];
    l.ym2 = src[e2m];
    l.yp2 = src[e2p];
    l.rr = R[ec];
    l.a0 = C0[ec];
    l.a1 = C1[ec];
    l.a1n = C1[e1p];
    l.a2 = C2[ec];
    l.a2n = C2[e2p];
    return l;
  }
  static __device__ __forceinline__ double step(const Loaded &l, int t, int T, double omega, double cf, double mu, double alpha) {
    return gvp_epoch_step(l.y0, l.ym1, l.yp1, l.ym2, l.yp2, l.a0, l.a1, l.a1n, l.a2, l.a2n, l.rr, t, T, omega, cf, mu, alpha);
  }
};

// ------------------------------------------------------------------------------------------------
// One workgroup per utterance (persistent loop over the call's utterances) runs all epochs; pv' (var - mu_v) couples all static
// dimensions once per epoch, so an utterance is not split.  Thread = (dimension d = tid % D, phase = tid / D) walks the frames
// phase, phase + NG, ... (NG = 512 / D): d is fastest across the lanes, a wave reads and writes whole rows of (T,D) arrays.
//   prologue, once per utterance: the two-pass moments of the solved trajectory, then ONE pass that rescales y by eq. (58) and
//     writes the stencil's coefficients -- the dependent gathers happen here and nowhere else;
//   epoch: the stencil's step from `src` into `dst`, kBatch frames per thread in flight on clamped addresses; the pass that
//     writes the new y accumulates its moments as shifted sums about the previous mean, reduced over the phases in a fixed
//     order (no atomics); then mean, var and coef for the next epoch.  Three barriers per epoch.
// NRES of the stencil's arrays are in LDS across the epochs, the others in the workspace (the first y then is the utterance's Y
// itself).  The arithmetic does not depend on NRES: an utterance's bits are the same in every batch.  After the last epoch the
// result is in Y: copied out of LDS, or, streamed, by starting in the buffer whose parity ends there.  Contraction is off: what
// is fused is written as fma.  nthr is blockDim.x, read by the kernel itself (where the compiler knows the workgroup size to be
// uniform); the other arguments are the kernel's.
// ------------------------------------------------------------------------------------------------
template <class Stencil, int NRES>
__device__ __forceinline__ void traj_gv_band(int nthr, const TrajUtt *utts, int n, int D, int64_t lds_arr, const double *q,
                                             const int64_t *mhat_all, const double *g_all, double *ws_gv, int64_t nframes,
                                             TrajGV gv) {
#pragma clang fp contract(off)
  static_assert(NRES == 0 || (NRES >= 2 && NRES <= Stencil::kArrays), "arrays resident in LDS");
  extern __shared__ double gsm[];
  const int DW = Stencil::kWindows * D;
  double *red = gsm;                       // [2][nthr]
  double *mean = red + 2 * nthr;           // [D]
  double *var = mean + D;                  // [D]
  double *coef = var + D;                  // [D]
  double *arr = coef + D;                  // [NRES][lds_arr]
  const int tid = threadIdx.x;
  const int NG = nthr / D, d = tid % D, ph = tid / D;
  const bool act = ph < NG;
  typedef typename BandPtr<(NRES >= 2)>::type YP;

  for (int u = blockIdx.x; u < n; u += gridDim.x) {
    const TrajUtt U = utts[u];
    const int T = U.T;
    if (T < 2) continue;                   // var() of one frame is undefined; the host rejects such calls
    const int64_t *mh = mhat_all + U.frame0;
    const double *g = g_all + U.frame0 * DW;
    gdouble *Yg = (gdouble *)U.Y;
    gdouble *wsu = (gdouble *)ws_gv + U.frame0 * D;
    // streamed, the ascent starts in the buffer from which `epochs` swaps end in Y
    YP src = band_sel<0, NRES>(arr, lds_arr, (gv.epochs & 1) ? wsu : Yg);
    YP dst = band_sel<1, NRES>(arr, lds_arr, (gv.epochs & 1) ? Yg : wsu);
    const Stencil S(arr, lds_arr, wsu, nframes * D);
    const double omega = 1.0 / (2.0 * (double)T);

    gv_moments(Yg, D, T, nthr, red, mean, var);
    // moments of the y just written from the shifted sums of the pass (traj_gv_kernel), then the gvgrad coefficients of the
    // next epoch, src/trajectory_gmmmap.jl:171-189: -2/T (pv' (var(y) - mu^v))
    auto finish = [&](double s1, double s2) {
      if (act) {
        red[ph * D + d] = s1;
        red[nthr + ph * D + d] = s2;
      }
      __syncthreads();
      if (tid < D) {
        double a1 = 0.0, a2 = 0.0;
        for (int k = 0; k < NG; ++k) {
          a1 += red[k * D + tid];
          a2 += red[nthr + k * D + tid];
        }
        mean[tid] += a1 / (double)T;
        var[tid] = (a2 - a1 * a1 / (double)T) / (double)(T - 1);       // Julia's var: corrected
      }
      __syncthreads();
      if (tid < D) {
        double s = 0.0;
        for (int j = 0; j < D; ++j) s = fma(gv.pv[j + (size_t)D * tid], var[j] - gv.muv[j], s);
        coef[tid] = -2.0 / (double)T * s;
      }
      __syncthreads();
    };

    // eq. (58): y <- sqrt(mu^v / var(y)) (y - mean) + mean, src/trajectory_gmmmap.jl:152; the stencil's coefficients
    {
      double s1 = 0.0, s2 = 0.0;
      if (act) {
        const double mu = mean[d], sc = sqrt(gv.muv[d] / var[d]);
#pragma unroll Stencil::kPrologueUnroll
        for (int t = ph; t < T; t += NG) {
          const size_t e = (size_t)t * D + d;
          const auto c = S.coefficients(t, T, D, d, q, mh, g);
          const double yn = sc * (Yg[e] - mu) + mu;
          src[e] = yn;
          S.store(e, c);
          const double dv = yn - mu;
          s1 += dv;
          s2 = fma(dv, dv, s2);
        }
      }
      finish(s1, s2);
    }

    for (int ep = 0; ep < gv.epochs; ++ep) {
      double s1 = 0.0, s2 = 0.0;
      if (act) {
        const double mu = mean[d], cf = coef[d];
        for (int t0 = ph; t0 < T; t0 += Stencil::kBatch * NG) {
          typename Stencil::Loaded l[Stencil::kBatch];
#pragma unroll
          for (int k = 0; k < Stencil::kBatch; ++k) {
            const int t = t0 + k * NG;
            l[k] = S.load(src, t < T ? t : T - 1, T, D, d);
          }
#pragma unroll
          for (int k = 0; k < Stencil::kBatch; ++k) {
            const int t = t0 + k * NG;
            if (t < T) {
              const double yn = Stencil::step(l[k], t, T, omega, cf, mu, gv.alpha);
              dst[(size_t)t * D + d] = yn;
              const double dv = yn - mu;
              s1 += dv;
              s2 = fma(dv, dv, s2);
            }
          }
        }
      }
      finish(s1, s2);       // (its first barrier is also the one between this epoch's reads of src and the next one's writes)
      const YP sw = src;
      src = dst;
      dst = sw;
    }
    if constexpr (NRES >= 2) {
      for (size_t e = tid; e < (size_t)T * D; e += nthr) Yg[e] = src[e];
      __syncthreads();                     // the next utterance writes the same LDS
    }
  }
}

}  // namespace vcmi
