// traj_gv.hip -- TrajectoryGVGMMMap (reference src/trajectory_gmmmap.jl:114-189): the handle, the three kernels of the
// global-variance ascent on solved trajectories (two for 2D <= 96, traj_gvw_kernel above that), and the host function that
// chooses between them (traj_internal.hpp: traj_gv_launch).  The ascent over diagonal conditional precisions: traj_gv_band.hip.
#include "traj_internal.hpp"
#include "traj_blk_prof.hpp"
#include "traj_gv_moments.hpp"
#include "traj_band_plan.hpp"
#include "host_linalg.hpp"
#include "hostpipe.hpp"

namespace vcmi {

// ------------------------------------------------------------------------------------------------
// Global-variance ascent, fvconvert(tgv::TrajectoryGVGMMMap, X), src/trajectory_gmmmap.jl:139-189.
// One workgroup per utterance runs all epochs:  y <- y + alpha * ( omega (r - P y) + gvgrad(y) ),  omega = 1/(2T),
// with P y = W' D^-1 W y applied as  u_t = [y_t ; (y_{t+1} - y_{t-1})/2]  ->  v_t = Q_mhat_t u_t  ->
// (P y)_t = vs_t + vd_{t-1}/2 - vd_{t+1}/2  (the stencil of W; W is never built) and r = W' D^-1 E from the g_t the
// solve already has.  v = Q u runs on v_mfma_f64_16x16x4 over tiles of 16 consecutive frames: wave i owns row tile i
// of Q; the tile's frames usually share one or two mixtures, so the product is accumulated over the DISTINCT
// mixtures of the tile with the B operand masked to that mixture's frames (exact: the other frames add 0).
// ------------------------------------------------------------------------------------------------
typedef double gv_d4 __attribute__((ext_vector_type(4)));
static constexpr int kGvNB = 8;   // 16-frame tiles per round of the GV product
static constexpr int kGvMaxKS = 24;   // k-steps of the widest supported feature vector (2D <= 96)

__global__ void __launch_bounds__(384)
traj_gv_kernel(const TrajUtt *__restrict__ utts, int n, int D, int M, int KS, const double *__restrict__ Qfrag,
               const int64_t *__restrict__ mhat_all, const double *__restrict__ g_all, double *__restrict__ ws_all,
               int64_t ws_stride, TrajGV gv) {
  extern __shared__ double gsm[];
  const int D2 = 2 * D, nthr = blockDim.x, NT = nthr >> 6;
  double *Ut = gsm;                        // [kGvNB][4*KS][16]  u of the tiles' frames, k-major
  double *red = Ut + (size_t)kGvNB * 4 * KS * 16;  // [2][nthr]
  double *mean = red + 2 * nthr;           // [D]
  double *var = mean + D;                  // [D]
  double *coef = var + D;                  // [D]
  int *cnt = reinterpret_cast<int *>(coef + D);   // [M] frames per mixture, then the fill cursor
  int *start = cnt + M;                           // [M] first slot of the mixture's (16-padded) segment
  __shared__ int tidx[16 * kGvNB];
  __shared__ int ntiles_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lcol = lane & 15, lgrp = lane >> 4;

  for (int u = blockIdx.x; u < n; u += gridDim.x) {
    const TrajUtt U = utts[u];
    const int T = U.T;
    if (T < 2) continue;                   // var() of one frame is undefined; the host rejects such calls
    const int64_t *mh = mhat_all + U.frame0;
    const double *g = g_all + U.frame0 * D2;
    gdouble *y = (gdouble *)U.Y;
    double *V = ws_all + (size_t)blockIdx.x * ws_stride;   // [T][2D]
    double *R = V + (size_t)T * D2;                        // [T][D]   r = W' D^-1 E
    int *perm = reinterpret_cast<int *>(R + (size_t)T * D); // frames grouped by mixture, segments padded to 16 with -1
    const double omega = 1.0 / (2.0 * (double)T);

    // frames grouped by mixture (the selection mhat is fixed over the epochs): every 16-frame tile of the product
    // below then has ONE mixture.  The order inside a group comes from atomics and is irrelevant: each frame's
    // product is computed independently.
    for (int m = tid; m < M; m += nthr) cnt[m] = 0;
    __syncthreads();
    for (int t = tid; t < T; t += nthr) atomicAdd(&cnt[(int)mh[t] - 1], 1);
    __syncthreads();
    if (tid == 0) {
      int pos = 0;
      for (int m = 0; m < M; ++m) {
        start[m] = pos;
        pos += (cnt[m] + 15) / 16 * 16;
        cnt[m] = 0;
      }
      ntiles_s = pos / 16;
    }
    __syncthreads();
    const int ntiles = ntiles_s;
    for (int e = tid; e < ntiles * 16; e += nthr) perm[e] = -1;
    __syncthreads();
    for (int t = tid; t < T; t += nthr) {
      const int m = (int)mh[t] - 1;
      perm[start[m] + atomicAdd(&cnt[m], 1)] = t;
    }

    // eq. (58): y <- sqrt(mu^v / var(y)) (y - mean) + mean, src/trajectory_gmmmap.jl:152; and r.
    // Every pass that writes y also accumulates the moments of what it writes (thread = (dimension d, frame group g),
    // the mapping of gv_moments): sum (y - c) and sum (y - c)^2 with the shift c = mean before the pass, so that
    // mean = c + S1/T, var = (S2 - S1^2/T)/(T-1) lose nothing to cancellation and the next epoch needs no pass of
    // its own over y for them.
    gv_moments(y, D, T, nthr, red, mean, var);
    const int NGm = nthr / D, dm = tid % D, gm = tid / D;
    auto finish_moments = [&](double s1, double s2) {
      if (gm < NGm) {
        red[gm * D + dm] = s1;
        red[nthr + gm * D + dm] = s2;
      }
      __syncthreads();
      if (tid < D) {
        double a1 = 0.0, a2 = 0.0;
        for (int k = 0; k < NGm; ++k) {
          a1 += red[k * D + tid];
          a2 += red[nthr + k * D + tid];
        }
        mean[tid] += a1 / (double)T;
        var[tid] = (a2 - a1 * a1 / (double)T) / (double)(T - 1);       // Julia's var: corrected
      }
      __syncthreads();
    };
    {
      double s1 = 0.0, s2 = 0.0;
      if (gm < NGm) {
        const double mu = mean[dm], sc = sqrt(gv.muv[dm] / var[dm]);
#pragma unroll 8
        for (int t = gm; t < T; t += NGm) {
          const size_t e = (size_t)t * D + dm;
          const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
          const double yo = y[e], g0 = g[(size_t)t * D2 + dm], g1 = g[(size_t)tm * D2 + D + dm], g2 = g[(size_t)tp * D2 + D + dm];
          const double yn = sc * (yo - mu) + mu;
          y[e] = yn;
          R[e] = (g0 + (t >= 1 ? 0.5 : 0.0) * g1) - (t + 1 < T ? 0.5 : 0.0) * g2;
          const double dv = yn - mu;
          s1 += dv;
          s2 = fma(dv, dv, s2);
        }
      }
      __syncthreads();
      finish_moments(s1, s2);
    }

    double afr[kGvMaxKS];
    int mcur = -1;
    for (int ep = 0; ep < gv.epochs; ++ep) {
      // gvgrad coefficients, src/trajectory_gmmmap.jl:171-189: -2/T (pv' (var(y) - mu^v)), times (y - mean) below;
      // mean and var of the current y come from the pass that wrote it
      if (tid < D) {
        double s = 0.0;
        for (int j = 0; j < D; ++j) s = fma(gv.pv[j + (size_t)D * tid], var[j] - gv.muv[j], s);
        coef[tid] = -2.0 / (double)T * s;
      }
      // v_t = Q_mhat_t u_t for every frame: kGvNB single-mixture tiles of 16 frames per round, so that the gathers of
      // y, the loads of the Q fragments and the barriers are paid once per 16*kGvNB frames
      for (int tile0 = 0; tile0 < ntiles; tile0 += kGvNB) {
        const int nb = (ntiles - tile0 < kGvNB) ? ntiles - tile0 : kGvNB;
        if (tid < 16 * nb) tidx[tid] = perm[tile0 * 16 + tid];
        __syncthreads();
        // u_t = [y_t ; (y_{t+1} - y_{t-1})/2]: two unconditional loads per element on clamped addresses with 0 / 1 / +-1/2
        // weights (a branch or a select on the loaded value would serialise the loads), eight elements in flight
#pragma unroll 8
        for (int e = tid; e < nb * 4 * KS * 16; e += nthr) {
          const int b = e / (4 * KS * 16), q = e - b * (4 * KS * 16);
          const int k = q >> 4, t = tidx[b * 16 + (q & 15)];
          const bool ok = t >= 0 && k < D2, st = k < D;
          const int tc = t >= 0 ? t : 0, kd = st ? (k < D ? k : 0) : (k < D2 ? k - D : 0);
          const int tp = tc + 1 < T ? tc + 1 : tc, tm = tc >= 1 ? tc - 1 : tc;
          const double a = y[(size_t)(st ? tc : tp) * D + kd], c = y[(size_t)(st ? tc : tm) * D + kd];
          const double wa = !ok ? 0.0 : (st ? 1.0 : (tc + 1 < T ? 0.5 : 0.0)), wc = (!ok || st) ? 0.0 : (tc >= 1 ? -0.5 : 0.0);
          Ut[e] = wa * a + wc * c;
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
          const int m = (int)mh[tidx[b * 16]] - 1;         // the tile's mixture (slot 0 of a tile is never padding)
          if (m != mcur) {                                 // Q fragments of this wave's row tile: all k-steps in flight at
            mcur = m;                                      // once, kept in registers while consecutive tiles share m
            const double *A = Qfrag + (((size_t)m * NT + wave) * KS) * 64 + lane;
#pragma unroll
            for (int ks = 0; ks < kGvMaxKS; ++ks) afr[ks] = (ks < KS) ? A[(size_t)ks * 64] : 0.0;
          }
          const double *Ub = Ut + (size_t)b * 4 * KS * 16;
          gv_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int ks = 0; ks < kGvMaxKS; ++ks)
            if (ks < KS) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[ks], Ub[(4 * ks + lgrp) * 16 + lcol], acc, 0, 0, 0);
          const int t = tidx[b * 16 + lcol];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * wave + lgrp + 4 * r;
            if (row < D2 && t >= 0) V[(size_t)t * D2 + row] = acc[r];
          }
        }
        __syncthreads();
      }
      // y <- y + alpha * ( omega (r - P y) + coef (y - mean) ), eq. (52), src/trajectory_gmmmap.jl:163-166
      double s1 = 0.0, s2 = 0.0;
      if (gm < NGm) {
        const double mu = mean[dm], cf = coef[dm];
#pragma unroll 8
        for (int t = gm; t < T; t += NGm) {
          const size_t e = (size_t)t * D + dm;
          const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
          const double vs = V[(size_t)t * D2 + dm], vm = V[(size_t)tm * D2 + D + dm], vp = V[(size_t)tp * D2 + D + dm];
          const double yy = y[e], rr = R[e];
          const double py = (vs + (t >= 1 ? 0.5 : 0.0) * vm) - (t + 1 < T ? 0.5 : 0.0) * vp;
          const double dy = omega * (rr - py) + cf * (yy - mu);
          const double yn = fma(gv.alpha, dy, yy);
          y[e] = yn;
          const double dv = yn - mu;
          s1 += dv;
          s2 = fma(dv, dv, s2);
        }
      }
      __syncthreads();
      finish_moments(s1, s2);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// traj_gv2_kernel: the same ascent with the product phase run by TWO teams of waves.  With one workgroup per CU the
// product rounds of traj_gv_kernel are a chain  gather (memory latency) -> barrier -> MFMA + store -> barrier;  here
// waves NT..2NT-1 gather the rows of y for round r+1 into the other of two LDS images of u while waves 0..NT-1 run the
// MFMAs of round r -- one barrier per round, and the streaming passes (scaling, update, moments) run on twice the
// threads.  The frame permutation and the tile mixtures live in LDS (no dependent global load in the rounds), which
// bounds the utterance length; longer utterances take traj_gv_kernel.
// ------------------------------------------------------------------------------------------------
static constexpr int kGv2NB = 4;     // 16-frame tiles per round
#ifndef VCMI_GV2_GB
#define VCMI_GV2_GB 12
#endif
static constexpr int kGv2GB = VCMI_GV2_GB;   // elements of u a gather thread has in flight
static constexpr int kGv2Threads = 768;   // 12 waves: NT = ceil(2D/16) MFMA waves, the rest gather (three waves per SIMD: 168 VGPRs)

__global__ void __launch_bounds__(kGv2Threads)
traj_gv2_kernel(const TrajUtt *__restrict__ utts, int n, int D, int M, int KS, int pcap, const double *__restrict__ Qfrag,
                const int64_t *__restrict__ mhat_all, const double *__restrict__ g_all, double *__restrict__ ws_all,
                int64_t ws_stride, TrajGV gv) {
  extern __shared__ double gsm[];
  const int D2 = 2 * D, nthr = blockDim.x, NT = (D2 + 15) / 16, nmf = 64 * NT, ngth = nthr - nmf;
  const int UTS = 4 * KS * 17, UTR = kGv2NB * UTS;
  double *Ut = gsm;                        // [2][kGv2NB][4*KS][17]  u of the tiles' frames, k-major, row stride 17
  double *red = Ut + 2 * (size_t)UTR;      // [2][nthr]
  double *mean = red + 2 * nthr;           // [D]
  double *var = mean + D;                  // [D]
  double *coef = var + D;                  // [D]
  int *cnt = reinterpret_cast<int *>(coef + D);   // [M] frames per mixture, then the fill cursor
  int *start = cnt + M;                           // [M] first slot of the mixture's (16-padded) segment
  int *perm = start + M;                          // [pcap] frames grouped by mixture, segments padded to 16 with -1
  int *tilem = perm + pcap;                       // [pcap / 16 + 1] mixture of every tile
  __shared__ int ntiles_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lcol = lane & 15, lgrp = lane >> 4;
  const bool gatherer = wave >= NT;
  const int gtid = tid - nmf;

  for (int u = blockIdx.x; u < n; u += gridDim.x) {
    const TrajUtt U = utts[u];
    const int T = U.T;
    if (T < 2) continue;                   // var() of one frame is undefined; the host rejects such calls
    const int64_t *mh = mhat_all + U.frame0;
    const double *g = g_all + U.frame0 * D2;
    gdouble *y = (gdouble *)U.Y;
    double *V = ws_all + (size_t)blockIdx.x * ws_stride;   // [T][2D]
    double *R = V + (size_t)T * D2;                        // [T][D]   r = W' D^-1 E
    const double omega = 1.0 / (2.0 * (double)T);

    // frames grouped by mixture (see traj_gv_kernel)
    for (int m = tid; m < M; m += nthr) cnt[m] = 0;
    __syncthreads();
    for (int t = tid; t < T; t += nthr) atomicAdd(&cnt[(int)mh[t] - 1], 1);
    __syncthreads();
    if (tid == 0) {
      int pos = 0;
      for (int m = 0; m < M; ++m) {
        start[m] = pos;
        pos += (cnt[m] + 15) / 16 * 16;
        cnt[m] = 0;
      }
      ntiles_s = pos / 16;
    }
    __syncthreads();
    const int ntiles = ntiles_s;
    for (int e = tid; e < ntiles * 16; e += nthr) perm[e] = -1;
    __syncthreads();
    for (int t = tid; t < T; t += nthr) {
      const int m = (int)mh[t] - 1;
      perm[start[m] + atomicAdd(&cnt[m], 1)] = t;
    }
    __syncthreads();
    for (int i = tid; i < ntiles; i += nthr) tilem[i] = (int)mh[perm[i * 16]] - 1;
    for (int e = tid; e < 2 * UTR; e += nthr) Ut[e] = 0.0;      // rows k >= 2D of the k-padding stay zero
    // elements of u a gather thread fetches in a round: e = gtid + i * ngth -> (frame slot e / 2D, k = e % 2D), k fastest
    // across threads; one division here, increments in the rounds
    const int gsl0 = gatherer ? gtid / D2 : 0, gk0 = gatherer ? gtid % D2 : 0, dsl = ngth / D2, dk = ngth % D2;

    // eq. (58) and r; every pass that writes y accumulates the moments of what it writes (see traj_gv_kernel)
    gv_moments(y, D, T, nthr, red, mean, var);
    const int NGm = nthr / D, dm = tid % D, gm = tid / D;
    auto finish_moments = [&](double s1, double s2) {
      if (gm < NGm) {
        red[gm * D + dm] = s1;
        red[nthr + gm * D + dm] = s2;
      }
      __syncthreads();
      if (tid < D) {
        double a1 = 0.0, a2 = 0.0;
        for (int k = 0; k < NGm; ++k) {
          a1 += red[k * D + tid];
          a2 += red[nthr + k * D + tid];
        }
        mean[tid] += a1 / (double)T;
        var[tid] = (a2 - a1 * a1 / (double)T) / (double)(T - 1);       // Julia's var: corrected
      }
      __syncthreads();
    };
    {
      double s1 = 0.0, s2 = 0.0;
      if (gm < NGm) {
        const double mu = mean[dm], sc = sqrt(gv.muv[dm] / var[dm]);
#pragma unroll 4
        for (int t = gm; t < T; t += NGm) {
          const size_t e = (size_t)t * D + dm;
          const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
          const double yo = y[e], g0 = g[(size_t)t * D2 + dm], g1 = g[(size_t)tm * D2 + D + dm], g2 = g[(size_t)tp * D2 + D + dm];
          const double yn = sc * (yo - mu) + mu;
          y[e] = yn;
          R[e] = (g0 + (t >= 1 ? 0.5 : 0.0) * g1) - (t + 1 < T ? 0.5 : 0.0) * g2;
          const double dv = yn - mu;
          s1 += dv;
          s2 = fma(dv, dv, s2);
        }
      }
      __syncthreads();
      finish_moments(s1, s2);
    }

    // gather of one round into an LDS image of u: two unconditional loads per element on clamped addresses, eight
    // elements in flight, 0 / 1 / +-1/2 weights applied on the way into LDS
    auto gather = [&](int r, double *Ub0) {
      const int tile0 = r * kGv2NB, total = 16 * kGv2NB * D2;
      int sl = gsl0, k = gk0;
      for (int e = gtid; e < total; e += kGv2GB * ngth) {
        double ya[kGv2GB], yc[kGv2GB];
        int tt[kGv2GB], oo[kGv2GB];
#pragma unroll
        for (int i = 0; i < kGv2GB; ++i) {
          const bool in = e + i * ngth < total;
          const int idx = tile0 * 16 + sl;
          const int t = (in && idx < ntiles * 16) ? perm[idx] : -1;
          tt[i] = (t < 0 ? -1 : t) | (k < D ? 0 : 1 << 30);         // frame and static / delta half
          oo[i] = in ? ((sl >> 4) * 4 * KS + k) * 17 + (sl & 15) : -1;
          const bool st = k < D;
          const int tc = t >= 0 ? t : 0, kd = st ? k : k - D;
          const int tp = tc + 1 < T ? tc + 1 : tc, tm = tc >= 1 ? tc - 1 : tc;
          ya[i] = y[(size_t)(st ? tc : tp) * D + kd];
          yc[i] = y[(size_t)(st ? tc : tm) * D + kd];
          sl += dsl;
          k += dk;
          if (k >= D2) {
            k -= D2;
            ++sl;
          }
        }
#pragma unroll
        for (int i = 0; i < kGv2GB; ++i)
          if (oo[i] >= 0) {
            const bool ok = tt[i] >= 0, st = (tt[i] & (1 << 30)) == 0;
            const int t = tt[i] & ~(1 << 30);
            const double wa = !ok ? 0.0 : (st ? 1.0 : (t + 1 < T ? 0.5 : 0.0)), wc = (!ok || st) ? 0.0 : (t >= 1 ? -0.5 : 0.0);
            Ub0[oo[i]] = wa * ya[i] + wc * yc[i];
          }
      }
    };

    double afr[kGvMaxKS];
    int mcur = -1;
    const int nrounds = (ntiles + kGv2NB - 1) / kGv2NB;
    BLK_PROF_T0();
    for (int ep = 0; ep < gv.epochs; ++ep) {
      // gvgrad coefficients, src/trajectory_gmmmap.jl:171-189: -2/T (pv' (var(y) - mu^v)), times (y - mean) below
      if (tid < D) {
        double s = 0.0;
        for (int j = 0; j < D; ++j) s = fma(gv.pv[j + (size_t)D * tid], var[j] - gv.muv[j], s);
        coef[tid] = -2.0 / (double)T * s;
      }
      // v_t = Q_mhat_t u_t for every frame
      if (gatherer) gather(0, Ut);
      __syncthreads();
      for (int r = 0; r < nrounds; ++r) {
        if (gatherer) {
          if (r + 1 < nrounds) gather(r + 1, Ut + (size_t)((r + 1) & 1) * UTR);
        } else {
          const double *Ub0 = Ut + (size_t)(r & 1) * UTR;
          const int tile0 = r * kGv2NB, nb = (ntiles - tile0 < kGv2NB) ? ntiles - tile0 : kGv2NB;
          for (int b = 0; b < nb; ++b) {
            const int m = tilem[tile0 + b];
            if (m != mcur) {                               // Q fragments of this wave's row tile, kept while tiles share m
              mcur = m;
              const double *A = Qfrag + (((size_t)m * NT + wave) * KS) * 64 + lane;
#pragma unroll
              for (int ks = 0; ks < kGvMaxKS; ++ks) afr[ks] = (ks < KS) ? A[(size_t)ks * 64] : 0.0;
            }
            const double *Ub = Ub0 + (size_t)b * UTS;
            gv_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < kGvMaxKS; ++ks)
              if (ks < KS) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[ks], Ub[(4 * ks + lgrp) * 17 + lcol], acc, 0, 0, 0);
            const int t = perm[(tile0 + b) * 16 + lcol];
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
              const int row = 16 * wave + lgrp + 4 * r4;
              if (row < D2 && t >= 0) V[(size_t)t * D2 + row] = acc[r4];
            }
          }
        }
        __syncthreads();
      }
      BLK_PROF(13);
      // y <- y + alpha * ( omega (r - P y) + coef (y - mean) ), eq. (52), src/trajectory_gmmmap.jl:163-166
      double s1 = 0.0, s2 = 0.0;
      if (gm < NGm) {
        const double mu = mean[dm], cf = coef[dm];
#pragma unroll 4
        for (int t = gm; t < T; t += NGm) {
          const size_t e = (size_t)t * D + dm;
          const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
          const double vs = V[(size_t)t * D2 + dm], vm = V[(size_t)tm * D2 + D + dm], vp = V[(size_t)tp * D2 + D + dm];
          const double yy = y[e], rr = R[e];
          const double py = (vs + (t >= 1 ? 0.5 : 0.0) * vm) - (t + 1 < T ? 0.5 : 0.0) * vp;
          const double dy = omega * (rr - py) + cf * (yy - mu);
          const double yn = fma(gv.alpha, dy, yy);
          y[e] = yn;
          const double dv = yn - mu;
          s1 += dv;
          s2 = fma(dv, dv, s2);
        }
      }
      __syncthreads();
      BLK_PROF(14);
      finish_moments(s1, s2);
      BLK_PROF(15);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// traj_gvw_kernel: the same ascent for feature vectors with more than six row tiles (2D > 96), where neither "one wave per
// row tile" nor "all k-steps of a tile in registers" holds.  Six MFMA waves and two gather waves; the streaming passes
// (moments, eq. (58), r, update) are those of traj_gv2_kernel on the (dimension, frame group) mapping, so D <= kGvwThreads.
//   product of a round (kGvwNB single-mixture tiles of 16 frames): work item = (row tile i, frame tile b), item i * kGvwNB + b;
//     the items are dealt to the MFMA waves in contiguous runs (a run mostly stays on one row tile, so its Q fragments are
//     loaded once for the frame tiles of the run), each item's 16 x 16 accumulator stays in registers over the whole k range:
//     at most kGvwItems per wave and pass, i.e. kGvwRowsPass row tiles per pass; wider models (2D > 192) take several passes
//     over the rows and gather u once per pass;
//   k range in chunks of kGvwKC k-steps: the LDS image of u holds ONE chunk of the round's tiles ([kGvwNB][4 kGvwKC][17]
//     doubles, 34 KB, two of them) whatever D is; the gather waves fill the image of step s + 1 while the MFMA waves multiply
//     step s, one barrier per step; the Q fragments of a chunk (kGvwKC registers) come from the handle's Qfrag image
//     ([M][NT][KS][64], built for every dimension by traj_prepare_model): one coalesced 512-byte load per k-step;
//   the frame permutation lives in LDS up to kGvwPermLds slots and in the workspace behind V and r beyond: LDS use depends on
//     neither D (beyond the 3 D moments) nor T.  The frames and the mixture of a round's tiles are left in LDS by the gather
//     of the round's first step (rt / rm), so the MFMA waves never read the permutation.
// The wide path always works in the static dimension D itself (no Dpad: the padded blocked solver ends at D = 46).
// ------------------------------------------------------------------------------------------------
static constexpr int kGvwNB = 4;          // 16-frame tiles per round
static constexpr int kGvwKC = 16;         // k-steps per chunk of the u image (64 columns)
static constexpr int kGvwThreads = 512;   // 8 waves, two per SIMD: 256 VGPRs
static constexpr int kGvwMfmaWaves = 6;
static constexpr int kGvwItems = 8;       // (row tile, frame tile) accumulators of an MFMA wave: 64 VGPRs
static constexpr int kGvwRowsPass = kGvwItems * kGvwMfmaWaves / kGvwNB;   // 12 row tiles per pass over the rows
static constexpr int kGvwGth = kGvwThreads - 64 * kGvwMfmaWaves;          // 256 gather threads
static constexpr int kGvwGB = kGvwNB * 16 * 4 * kGvwKC / kGvwGth;         // 32 elements of u per gather thread and step ...
static constexpr int kGvwGF = 16;                                         // ... 16 of them in flight
static constexpr int kGvwPermLds = 1024;  // slots of the frame permutation kept in LDS (4 KB: utterances of about 1000 frames)
static_assert(kGvwGth % 64 == 0 && kGvwGB * kGvwGth == kGvwNB * 16 * 4 * kGvwKC && 4 * kGvwKC == 64 && kGvwGB % kGvwGF == 0,
              "gather mapping of traj_gvw_kernel");

__global__ void __launch_bounds__(kGvwThreads)
traj_gvw_kernel(const TrajUtt *__restrict__ utts, int n, int D, int M, int NT, int KS, int perm_lds, const double *__restrict__ Qfrag,
                const int64_t *__restrict__ mhat_all, const double *__restrict__ g_all, double *__restrict__ ws_all,
                int64_t ws_stride, TrajGV gv) {
  extern __shared__ double gsm[];
  const int D2 = 2 * D, nthr = blockDim.x;
  constexpr int UTS = 4 * kGvwKC * 17, UTR = kGvwNB * UTS;
  double *Ut = gsm;                        // [2][kGvwNB][4*kGvwKC][17]  one k chunk of u of the tiles' frames, k-major, row stride 17
  double *red = Ut + 2 * (size_t)UTR;      // [2][nthr]
  double *mean = red + 2 * nthr;           // [D]
  double *var = mean + D;                  // [D]
  double *coef = var + D;                  // [D]
  int *cnt = reinterpret_cast<int *>(coef + D);   // [M] frames per mixture, then the fill cursor
  int *start = cnt + M;                           // [M] first slot of the mixture's (16-padded) segment
  int *perm_s = start + M;                        // [perm_lds] the frame permutation, when it fits
  __shared__ int ntiles_s;
  __shared__ int rt[2][16 * kGvwNB];       // frames of the round's tile slots (-1: padding), by round parity
  __shared__ int rm[2][kGvwNB];            // mixture of the round's tiles (-1: no such tile)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lcol = lane & 15, lgrp = lane >> 4;
  const bool gatherer = wave >= kGvwMfmaWaves;
  const int gtid = tid - 64 * kGvwMfmaWaves;
  const int NC = (KS + kGvwKC - 1) / kGvwKC;                   // k chunks ...
  const int KCe = (KS + NC - 1) / NC;                          // ... of KCe <= kGvwKC k-steps each (even shares: 25 -> 13 + 12)
  const int NP = (NT + kGvwRowsPass - 1) / kGvwRowsPass;       // passes over the row tiles ...
  const int RP = (NT + NP - 1) / NP;                           // ... of RP row tiles each (even shares: 13 -> 7 + 6)
  const int SPR = NP * NC;                                     // steps per round

  for (int u = blockIdx.x; u < n; u += gridDim.x) {
    const TrajUtt U = utts[u];
    const int T = U.T;
    if (T < 2) continue;                   // var() of one frame is undefined; the host rejects such calls
    const int64_t *mh = mhat_all + U.frame0;
    const double *g = g_all + U.frame0 * D2;
    gdouble *y = (gdouble *)U.Y;
    double *V = ws_all + (size_t)blockIdx.x * ws_stride;   // [T][2D]
    double *R = V + (size_t)T * D2;                        // [T][D]   r = W' D^-1 E
    // frames grouped by mixture, segments padded to 16 with -1: at most T + 15 min(M, T) slots
    int *perm = perm_lds > 0 ? perm_s : reinterpret_cast<int *>(R + (size_t)T * D);
    const double omega = 1.0 / (2.0 * (double)T);

    // frames grouped by mixture (see traj_gv_kernel)
    for (int m = tid; m < M; m += nthr) cnt[m] = 0;
    __syncthreads();
    for (int t = tid; t < T; t += nthr) atomicAdd(&cnt[(int)mh[t] - 1], 1);
    __syncthreads();
    if (tid == 0) {
      int pos = 0;
      for (int m = 0; m < M; ++m) {
        start[m] = pos;
        pos += (cnt[m] + 15) / 16 * 16;
        cnt[m] = 0;
      }
      ntiles_s = pos / 16;
    }
    __syncthreads();
    const int ntiles = ntiles_s;
    for (int e = tid; e < ntiles * 16; e += nthr) perm[e] = -1;
    __syncthreads();
    for (int t = tid; t < T; t += nthr) {
      const int m = (int)mh[t] - 1;
      perm[start[m] + atomicAdd(&cnt[m], 1)] = t;
    }
    __syncthreads();

    // eq. (58) and r; every pass that writes y accumulates the moments of what it writes (see traj_gv_kernel)
    gv_moments(y, D, T, nthr, red, mean, var);
    const int NGm = nthr / D, dm = tid % D, gm = tid / D;
    auto finish_moments = [&](double s1, double s2) {
      if (gm < NGm) {
        red[gm * D + dm] = s1;
        red[nthr + gm * D + dm] = s2;
      }
      __syncthreads();
      if (tid < D) {
        double a1 = 0.0, a2 = 0.0;
        for (int k = 0; k < NGm; ++k) {
          a1 += red[k * D + tid];
          a2 += red[nthr + k * D + tid];
        }
        mean[tid] += a1 / (double)T;
        var[tid] = (a2 - a1 * a1 / (double)T) / (double)(T - 1);       // Julia's var: corrected
      }
      __syncthreads();
    };
    {
      double s1 = 0.0, s2 = 0.0;
      if (gm < NGm) {
        const double mu = mean[dm], sc = sqrt(gv.muv[dm] / var[dm]);
#pragma unroll 4
        for (int t = gm; t < T; t += NGm) {
          const size_t e = (size_t)t * D + dm;
          const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
          const double yo = y[e], g0 = g[(size_t)t * D2 + dm], g1 = g[(size_t)tm * D2 + D + dm], g2 = g[(size_t)tp * D2 + D + dm];
          const double yn = sc * (yo - mu) + mu;
          y[e] = yn;
          R[e] = (g0 + (t >= 1 ? 0.5 : 0.0) * g1) - (t + 1 < T ? 0.5 : 0.0) * g2;
          const double dv = yn - mu;
          s1 += dv;
          s2 = fma(dv, dv, s2);
        }
      }
      __syncthreads();
      finish_moments(s1, s2);
    }

    // gather of step (round r, k chunk c) into an LDS image of u: thread -> one column k of the chunk and every second slot of
    // the round's 64 (k fastest across the threads: the reads of y run along its rows); two unconditional loads per element
    // on clamped addresses, sixteen elements in flight, 0 / 1 / +-1/2 weights applied on the way into LDS.  Every element of the image is
    // written (zero for padding slots, for k >= 2D and for the columns behind the chunk's KCe k-steps).  first: also leave the slots' frames and the tiles' mixtures in rt / rm.
    auto gather = [&](int r, int c, bool first, double *Ub0) {
      const int kk = gtid & 63, k = 4 * KCe * c + kk, sl0 = gtid >> 6;
      const bool st = k < D, kin = k < D2 && kk < 4 * KCe;
      const int kd = st ? k : (kin ? k - D : 0);
      constexpr int SLW = kGvwGth / 64;      // slots between two elements of a thread
      for (int i0 = 0; i0 < kGvwGB; i0 += kGvwGF) {
        double ya[kGvwGF], yc[kGvwGF];
        int tt[kGvwGF];
#pragma unroll
        for (int i = 0; i < kGvwGF; ++i) {
          const int sl = sl0 + SLW * (i0 + i), idx = r * (16 * kGvwNB) + sl;
          const int t = idx < ntiles * 16 ? perm[idx] : -1;
          tt[i] = t;
          const int tc = t >= 0 ? t : 0;
          const int tp = tc + 1 < T ? tc + 1 : tc, tm = tc >= 1 ? tc - 1 : tc;
          ya[i] = y[(size_t)(st ? tc : tp) * D + kd];
          yc[i] = y[(size_t)(st ? tc : tm) * D + kd];
        }
#pragma unroll
        for (int i = 0; i < kGvwGF; ++i) {
          const int sl = sl0 + SLW * (i0 + i), t = tt[i];
          const bool ok = t >= 0 && kin;
          const double wa = !ok ? 0.0 : (st ? 1.0 : (t + 1 < T ? 0.5 : 0.0)), wc = (!ok || st) ? 0.0 : (t >= 1 ? -0.5 : 0.0);
          Ub0[((sl >> 4) * 4 * kGvwKC + kk) * 17 + (sl & 15)] = wa * ya[i] + wc * yc[i];
          if (first && kk == 0) {
            rt[r & 1][sl] = t;
            if ((sl & 15) == 0) rm[r & 1][sl >> 4] = t >= 0 ? (int)mh[t] - 1 : -1;     // (slot 0 of a tile is never padding)
          }
        }
      }
    };

    const int nrounds = (ntiles + kGvwNB - 1) / kGvwNB;
    const int nsteps = nrounds * SPR;
    for (int ep = 0; ep < gv.epochs; ++ep) {
      // gvgrad coefficients, src/trajectory_gmmmap.jl:171-189: -2/T (pv' (var(y) - mu^v)), times (y - mean) below
      if (tid < D) {
        double s = 0.0;
        for (int j = 0; j < D; ++j) s = fma(gv.pv[j + (size_t)D * tid], var[j] - gv.muv[j], s);
        coef[tid] = -2.0 / (double)T * s;
      }
      // v_t = Q_mhat_t u_t for every frame.  The two teams run loops of their own (the accumulators are live in the MFMA
      // waves' loop only) and meet at one barrier per step: both loops execute exactly nsteps of them.
      if (gatherer) {
        gather(0, 0, true, Ut);
        __syncthreads();
        for (int s = 0; s < nsteps; ++s) {
          if (s + 1 < nsteps) {
            const int r1 = (s + 1) / SPR, sr1 = s + 1 - r1 * SPR;
            gather(r1, sr1 % NC, sr1 == 0, Ut + (size_t)((s + 1) & 1) * UTR);
          }
          __syncthreads();
        }
      } else {
        __syncthreads();
        gv_d4 acc[kGvwItems];
        for (int s = 0; s < nsteps; ++s) {
          const int r = s / SPR, sr = s - r * SPR, pass = sr / NC, c = sr - pass * NC;
          const double *Ub0 = Ut + (size_t)(s & 1) * UTR;
          const int i0 = pass * RP;
          const int nitems = (NT - i0 < RP ? NT - i0 : RP) * kGvwNB;
          const int per = (nitems + kGvwMfmaWaves - 1) / kGvwMfmaWaves, q0 = wave * per;
          double afr[kGvwKC];
          int icur = -1, mcur = -1;        // (the fragments in afr belong to this chunk: nothing is kept across steps)
#pragma unroll
          for (int j = 0; j < kGvwItems; ++j) {
            const int q = q0 + j;
            if (c == 0) acc[j] = gv_d4{0.0, 0.0, 0.0, 0.0};
            const int i = i0 + q / kGvwNB, b = q % kGvwNB;
            const int m = (j < per && q < nitems) ? rm[r & 1][b] : -1;
            if (m >= 0) {
              if (i != icur || m != mcur) {                    // Q fragments of (mixture, row tile, this chunk)
                icur = i;
                mcur = m;
                // every load unconditional, on a clamped k-step (a branch per load would serialise them); what lies beyond the
                // chunk is not multiplied, and the k-steps a last chunk repeats meet the zero rows k >= 2D of u
                const double *A = Qfrag + (((size_t)m * NT + i) * KS) * 64 + lane;
#pragma unroll
                for (int ks = 0; ks < kGvwKC; ++ks) {
                  const int kg = KCe * c + ks;
                  afr[ks] = A[(size_t)(kg < KS ? kg : KS - 1) * 64];
                }
              }
              const double *Ub = Ub0 + (size_t)b * UTS;
              gv_d4 a = acc[j];
#pragma unroll
              for (int k0 = 0; k0 < kGvwKC; k0 += 8) {         // eight operands of u in flight
                double bfr[8];
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) bfr[ks] = Ub[(4 * (k0 + ks) + lgrp) * 17 + lcol];
#pragma unroll
                for (int ks = 0; ks < 8; ++ks)
                  if (k0 + ks < KCe) a = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[k0 + ks], bfr[ks], a, 0, 0, 0);
              }
              acc[j] = a;
              if (c == NC - 1) {
                const int t = rt[r & 1][b * 16 + lcol];
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                  const int row = 16 * i + lgrp + 4 * r4;
                  if (row < D2 && t >= 0) V[(size_t)t * D2 + row] = a[r4];
                }
              }
            }
          }
          __syncthreads();
        }
      }
      // y <- y + alpha * ( omega (r - P y) + coef (y - mean) ), eq. (52), src/trajectory_gmmmap.jl:163-166
      double s1 = 0.0, s2 = 0.0;
      if (gm < NGm) {
        const double mu = mean[dm], cf = coef[dm];
#pragma unroll 4
        for (int t = gm; t < T; t += NGm) {
          const size_t e = (size_t)t * D + dm;
          const int tm = t >= 1 ? t - 1 : t, tp = t + 1 < T ? t + 1 : t;
          const double vs = V[(size_t)t * D2 + dm], vm = V[(size_t)tm * D2 + D + dm], vp = V[(size_t)tp * D2 + D + dm];
          const double yy = y[e], rr = R[e];
          const double py = (vs + (t >= 1 ? 0.5 : 0.0) * vm) - (t + 1 < T ? 0.5 : 0.0) * vp;
          const double dy = omega * (rr - py) + cf * (yy - mu);
          const double yn = fma(gv.alpha, dy, yy);
          y[e] = yn;
          const double dv = yn - mu;
          s1 += dv;
          s2 = fma(dv, dv, s2);
        }
      }
      __syncthreads();
      finish_moments(s1, s2);
    }
  }
}

// LDS of traj_gvw_kernel: two images of one k chunk, the reduction rows, the 3 D moments, the per-mixture counters and, when it
// fits, the permutation
static size_t gvw_lds_bytes(int D, int M, int perm_lds) {
  return ((size_t)2 * kGvwNB * 4 * kGvwKC * 17 + 2 * kGvwThreads + 3 * (size_t)D) * sizeof(double) + (2 * (size_t)M + (size_t)perm_lds) * sizeof(int);
}

static int traj_gvw_launch(vcmi_traj *t, const TrajSolvePlan &p, const TrajGV &gv, hipStream_t st) {
  const int D = t->D;
  if (D > kGvwThreads) return fail(VCMI_ERR_ARG, "TrajectoryGVGMMMap: static dimension %d beyond %d", D, kGvwThreads);
  // the workspace of a workgroup: V (2D,T) + r (D,T) and, behind them, room for the permutation (at most 16 T ints) -- the
  // plan of a call with GV reserves it (traj_solve_plan); checked here because this kernel writes all three
  const int64_t need = (int64_t)p.Tmax * 3 * D + (17 * (int64_t)p.Tmax + 1) / 2 + 16;
  if (p.ws_stride < need) return fail(VCMI_ERR_ARG, "TrajectoryGVGMMMap: workspace stride %lld below %lld", (long long)p.ws_stride, (long long)need);
  const int pcap = ((p.Tmax + 15) / 16 + t->M) * 16;       // slots the longest utterance can need
  const int perm_lds = pcap <= kGvwPermLds ? pcap : 0;
  const size_t shmem = gvw_lds_bytes(D, t->M, perm_lds);
  if (shmem > 160 * 1024 - 256) return fail(VCMI_ERR_ARG, "TrajectoryGVGMMMap: %d mixtures at dimension %d do not fit LDS", t->M, t->D2);
  VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(traj_gvw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(traj_gvw_kernel, dim3(p.grid), dim3(kGvwThreads), shmem, st, p.du, p.n, D, t->M, t->NT, t->KS, perm_lds, t->Qfrag.p,
                     t->mhat.p, t->gbuf.p, t->ws.p, p.ws_stride, gv);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// workspace: V (2D,T) + r (D,T) <= the panel area
int traj_gv_launch(vcmi_traj *t, const TrajSolvePlan &p, const TrajGV &gv, hipStream_t st) {
  const int D = t->D;
  if (t->NT > 6) return traj_gvw_launch(t, p, gv, st);      // 2D > 96: several row tiles per wave, k range in chunks
  // two-team kernel when the frame permutation of the longest utterance fits in LDS beside the two images of u
  const int pcap = ((p.Tmax + 15) / 16 + t->M) * 16;
  const int nthr2 = kGv2Threads;
  const size_t shmem2 = ((size_t)2 * kGv2NB * 4 * t->KS * 17 + 2 * nthr2 + 3 * (size_t)D) * sizeof(double) +
                        (2 * (size_t)t->M + (size_t)pcap + (size_t)pcap / 16 + 2) * sizeof(int);
  if (shmem2 <= 160 * 1024 - 256 && t->NT <= 6 && !debug_flag(kDbgGvOneTeam)) {
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(traj_gv2_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)shmem2));
    hipLaunchKernelGGL(traj_gv2_kernel, dim3(p.grid), dim3(nthr2), shmem2, st, p.du, p.n, D, t->M, t->KS, pcap, t->Qfrag.p, t->mhat.p,
                       t->gbuf.p, t->ws.p, p.ws_stride, gv);
  } else {
    const int nthr = 64 * t->NT;
    const size_t shmem = ((size_t)kGvNB * 4 * t->KS * 16 + 2 * nthr + 3 * (size_t)D) * sizeof(double) + 2 * (size_t)t->M * sizeof(int);
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(traj_gv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)shmem));
    hipLaunchKernelGGL(traj_gv_kernel, dim3(p.grid), dim3(nthr), shmem, st, p.du, p.n, D, t->M, t->KS, t->Qfrag.p, t->mhat.p, t->gbuf.p,
                       t->ws.p, p.ws_stride, gv);
  }
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

#ifdef TRAJ_BLK_PROF
void traj_gv_prof_dump(hipStream_t st) {
  long long h[32];
  blk_prof_fetch(h, st);
  fprintf(stderr, "blk_prof cycles, gv kernel: product phase %lld, update %lld, moments %lld\n", h[13], h[14], h[15]);
}
#endif

int trajgv_args(const vcmi_trajgv *h, int64_t n, const int64_t *T, int epochs, TrajGV *gv) {
  if (!h) return fail(VCMI_ERR_ARG, "TrajectoryGVGMMMap: NULL handle");
  if (epochs < 0) return fail(VCMI_ERR_ARG, "TrajectoryGVGMMMap: negative epoch count");
  if (h->t->D > kGvwThreads)    // (the arg-max of the trajectory converter itself ends at 2D = 320)
    return fail(VCMI_ERR_ARG, "TrajectoryGVGMMMap: static dimension %d beyond %d", h->t->D, kGvwThreads);
  if (h->t->em_iters > 0)    // the GV ascent groups frames by mhat[t] <= M and reads Qfrag: no blended precisions
    return fail(VCMI_ERR_ARG, "TrajectoryGVGMMMap: the trajectory converter has EM re-estimation switched on (vcmi_traj_set_em)");
  if (h->diag) {      // a handle of vcmi_trajgv_create_diag runs traj_gvd_kernel, which reads q alone
    if (h->t->precision != VCMI_TRAJ_PRECISION_DIAG)
      return fail(VCMI_ERR_ARG, "DiagTrajectoryGVGMMMap: the trajectory converter has been switched to full conditional precisions "
                                "(vcmi_traj_set_precision): switch it back, or make the handle with vcmi_trajgv_create");
    if (h->t->D > kGvdThreads) return fail(VCMI_ERR_ARG, "DiagTrajectoryGVGMMMap: static dimension %d beyond %d", h->t->D, kGvdThreads);
  } else if (h->t->precision == VCMI_TRAJ_PRECISION_DIAG)    // ... and it multiplies by the full Q_m
    return fail(VCMI_ERR_ARG, "TrajectoryGVGMMMap: the trajectory converter has diagonal conditional precisions (vcmi_traj_set_precision); "
                              "vcmi_trajgv_create_diag makes a handle for such a converter");
  for (int64_t u = 0; T && u < n; ++u)
    if (T[u] == 1) return fail(VCMI_ERR_DIM, "TrajectoryGVGMMMap: the variance of a one-frame trajectory is undefined");
  gv->muv = h->muv.p;
  gv->pv = h->pv.p;
  gv->epochs = epochs;
  return VCMI_OK;
}

}  // namespace vcmi

using namespace vcmi;

// ---- TrajectoryGVGMMMap, src/trajectory_gmmmap.jl:114-189 ----------------------------------------
// bdiag: vcmi_trajgv_create_bdiag -- a cross-diagonal converter only, with two windows (the handle of vcmi_trajgv_create_diag) or
// three (traj_gv_band.hip)
static int trajgv_create(vcmi_traj *t, const double *muv, const double *sigmavv, bool diag, vcmi_trajgv **out, bool bdiag = false) {
  const char *who = bdiag ? "vcmi_trajgv_create_bdiag" : diag ? "vcmi_trajgv_create_diag" : "vcmi_trajgv_create";
  if (!t || !muv || !sigmavv || !out) return fail(VCMI_ERR_ARG, "%s: NULL argument", who);
  *out = nullptr;
  if (bdiag && !t->b)
    return fail(VCMI_ERR_ARG, "vcmi_trajgv_create_bdiag: the trajectory converter is not one of vcmi_traj_create_bdiag[_windows]: "
                              "vcmi_trajgv_create or vcmi_trajgv_create_diag makes the handle for it");
  if (diag && !bdiag) VCMI_TRY(traj_two_windows_only(t, who, "the GV ascent"));     // (traj_gvd_kernel's gradient is the two-window stencil)
  if (diag && t->precision != VCMI_TRAJ_PRECISION_DIAG)
    return fail(VCMI_ERR_ARG, "vcmi_trajgv_create_diag: the trajectory converter has full conditional precisions "
                              "(vcmi_traj_set_precision): vcmi_trajgv_create makes the handle for it");
  if (diag && t->D > kGvdThreads) return fail(VCMI_ERR_ARG, "DiagTrajectoryGVGMMMap: static dimension %d beyond %d", t->D, kGvdThreads);
  const int D = t->D;
  for (int d = 0; d < D; ++d)
    if (muv[d] < 0.0) return fail(VCMI_ERR_ARG, "TrajectoryGVGMMMap: the GV mean must be non-negative");   // the @assert of :124
  std::vector<double> S((size_t)D * D), P((size_t)D * D);
  for (int r = 0; r < D; ++r)
    for (int c = 0; c < D; ++c) S[(size_t)r * D + c] = sigmavv[r + (size_t)D * c];
  if (!la::inverse(S.data(), D, P.data())) return fail(VCMI_ERR_NOT_PD, "TrajectoryGVGMMMap: the GV covariance is singular");
  std::vector<double> Pj((size_t)D * D);                       // back to the Julia memory image
  for (int r = 0; r < D; ++r)
    for (int c = 0; c < D; ++c) Pj[r + (size_t)D * c] = P[(size_t)r * D + c];
  vcmi_trajgv *h = new (std::nothrow) vcmi_trajgv();
  if (!h) return fail(VCMI_ERR_OOM, "out of host memory");
  h->t = t;
  h->diag = diag;
  int rc = VCMI_OK;
  if ((rc = h->muv.alloc(D)) || (rc = h->pv.alloc((size_t)D * D))) {
    delete h;
    return rc;
  }
  hipError_t e = upload_now_hip(h->muv.p, muv, sizeof(double) * D);
  if (e == hipSuccess) e = upload_now_hip(h->pv.p, Pj.data(), sizeof(double) * D * D);
  if (e != hipSuccess) {
    delete h;
    return fail(VCMI_ERR_HIP, "TrajectoryGVGMMMap: upload failed: %s", hipGetErrorString(e));
  }
  h->h_muv.assign(muv, muv + D);
  h->h_pv = Pj;
  *out = h;
  return VCMI_OK;
}

extern "C" int vcmi_trajgv_create(vcmi_traj *t, const double *muv, const double *sigmavv, vcmi_trajgv **out) {
  return trajgv_create(t, muv, sigmavv, false, out);
}

// ... over a converter with diagonal conditional precisions (vcmi_traj_set_precision, vcmi_traj_create_bdiag): traj_gv_band.hip
extern "C" int vcmi_trajgv_create_diag(vcmi_traj *t, const double *muv, const double *sigmavv, vcmi_trajgv **out) {
  return trajgv_create(t, muv, sigmavv, true, out);
}

// ... over a converter made straight from a cross-diagonal model, with two windows (the handle above, bit for bit) or three
// (traj_gv_band.hip: traj_gvp_kernel)
extern "C" int vcmi_trajgv_create_bdiag(vcmi_traj *t, const double *muv, const double *sigmavv, vcmi_trajgv **out) {
  return trajgv_create(t, muv, sigmavv, true, out, true);
}

extern "C" int vcmi_trajgv_destroy(vcmi_trajgv *h) {
  delete h;
  return VCMI_OK;
}
