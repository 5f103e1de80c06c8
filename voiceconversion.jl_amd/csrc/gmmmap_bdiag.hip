// gmmmap_bdiag.hip -- frame-by-frame conversion with a CROSS-DIAGONAL ("block_diag") joint GMM, MI355X (gfx950): the
// vcmi_bdmap handle and every vcmi_bdmap_* / vcmi_vc_bdmap* entry (include/vcmi.h).
//
// The model (Toda, Black, Tokuda 2007; what train_gmm(covariance_type="block_diag") returns): the four blocks of the joint
// covariance are diagonal, so per mixture m and dimension d
//   l_tm = cst_m - 1/2 sum_d (x_dt - mux_dm)^2 / vx_dm          (CENTRED: DESIGN 3.1-BDIAG, 3.3c)
//   p_tm = softmax_m l_tm                                        (max-shifted; cst_m = -inf for w_m <= 0: p = 0 exactly)
//   y_dt = sum_m p_tm (muy_dm + a_dm (x_dt - mux_dm)),  a = c / vx
// about 6 D M FP64 vector operations per frame where the dense converter issues M (3 D^2 + 6 D) flop.
//
// One kernel, four modes (0 fvconvert, 1 predict_proba, 2 predict, 3 the arg-max + g_t pass of trajectory conversion straight
// from the model: below), one launch per call.  A workgroup of eight waves takes
// FB consecutive frames (64; 32 where the two tiles below would not fit the LDS of a CU), lane = frame:
//   stage    the frames, read once, transposed into LDS: xs[d][frame]
//   phase 1  wave w takes the mixtures 4 w .. 4 w + 3, then + 32, ...: one LDS read of x_d serves four mixtures, whose
//            parameters are wave-uniform (scalar loads, four dimensions of a mixture per load) at FB = 64; l goes to
//            LDS, L[m][frame]
//   phase 2  thread (part, frame): maximum, sum and quotient over the mixtures part, part + NP, ..., the NP partial results
//            of a frame combined through LDS in a fixed order (mode 2: the first maximum instead)
//   phase 3  wave w takes the dimensions 2 w, 2 w + 1, then + 16, ...: y over all mixtures, the posteriors read from LDS once
//            per pair of dimensions; y replaces x in xs (each element is read and written by the same lane)
//   store    y (or P, or the index), written once, consecutive lanes on consecutive addresses
// Mode 3 (vcmi_traj_create_bdiag) shares the staging, phase 1 and mode 2's first-maximum reduction; the index
// goes to LDS as well as to HBM, and in place of phase 3
//   phase 3t thread (part, frame): g_d = q_d,mhat (mu_y + a (x_d - mu_x)) for the dimensions part, part + NP, ... and the frame's
//            OWN mixture only -- the mixture is per lane now, so the [mu_x, a, mu_y, q] row of (mhat, d) is a 32-byte gather
//            from prm4; the lanes of a wave are consecutive frames, which mostly share a mixture: one or two cache lines per load
// then the same store.
// Nothing per (frame, mixture) goes to HBM.  Every index is a function of (D, M, T, ld) and the thread alone; a frame's
// arithmetic does not depend on its lane, its workgroup or the other frames: no atomics, same bits in every call.
#include "gmmmap_bdiag_handle.hpp"
#include "gmmmap_bdiag_prepare.hpp"
#include "hostpipe.hpp"
#include "postf.hpp"

#include <cmath>

namespace vcmi {

static constexpr int kBdmThreads = 512;
static constexpr size_t kBdmLdsBudget = 160 * 1024;
// chunks of the host pipeline hold at least this many frames (as the dense converter's: one full round of workgroups)
static constexpr int64_t kBdmMinChunkFrames = 98304;

typedef double bdm_d4 __attribute__((ext_vector_type(4)));

static size_t bdmap_lds_bytes(int DP, int M, int FB) {
  return ((size_t)DP * (FB + 1) + (size_t)M * FB + kBdmThreads) * sizeof(double) + kBdmThreads * sizeof(int);
}

// the tile in xs, written once: consecutive lanes on consecutive addresses
template <int FB>
__device__ __forceinline__ void bdmap_store_tile(const double *xs, double *Y, int64_t ldy, int64_t f0, int nf, int D, int DP) {
  for (int i = threadIdx.x; i < FB * DP; i += kBdmThreads) {
    const int yf = i / DP, d = i - yf * DP;
    if (yf < nf && d < D) Y[(f0 + yf) * ldy + d] = xs[d * (FB + 1) + yf];
  }
}

template <int MODE, int FB>
__global__ void __launch_bounds__(kBdmThreads)
bdmap_kernel(const double *X, int64_t ldx, int64_t T, int D, int DP, int M, const double *__restrict__ prm1,
             const double *__restrict__ prm3, const double *__restrict__ cst, void *out, int64_t ldy, int64_t *mhat) {
  extern __shared__ double lds[];
  constexpr int RS = FB + 1, NS = 64 / FB, NP = kBdmThreads / FB, NW = kBdmThreads / 64;
  double *xs = lds;                               // [DP][RS]
  double *L = xs + (size_t)DP * RS;               // [M][FB]
  double *red = L + (size_t)M * FB;               // [NP][FB]
  int *redi = reinterpret_cast<int *>(red + kBdmThreads);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = lane & (FB - 1), sub = lane / FB;
  const int64_t f0 = (int64_t)blockIdx.x * FB;
  const int nf = (int)((T - f0 < FB) ? T - f0 : FB);

  for (int i = tid; i < FB * DP; i += kBdmThreads) {
    const int fr = i / DP, d = i - fr * DP;
    xs[d * RS + fr] = (fr < nf && d < D) ? X[(f0 + fr) * ldx + d] : 0.0;
  }
  __syncthreads();

  // phase 1
  for (int mw = 4 * NS * wave; mw < M; mw += 4 * NS * NW) {
    int mb = mw + 4 * sub;
    if (FB == 64) mb = __builtin_amdgcn_readfirstlane(mb);
    const double *p[4];
    double q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = prm1 + (size_t)((mb + j < M) ? mb + j : M - 1) * DP * kBdmapPrm1;
    // four dimensions at a time (DP is a multiple of four; the padding rows are zeros on both sides): eight consecutive
    // doubles of a mixture per load; a mixture's sum runs over d in ascending order
    for (int d = 0; d < DP; d += 4) {
      double x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = xs[(d + k) * RS + f];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double *pj = p[j] + d * kBdmapPrm1;
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

  // phase 2
  const int fr = tid & (FB - 1), part = tid / FB;
  if (MODE >= 2) {
    double best = -INFINITY;
    int bi = M;
    for (int m = part; m < M; m += NP) {
      const double v = L[m * FB + fr];
      if (v > best) {
        best = v;
        bi = m;
      }
    }
    red[part * FB + fr] = best;
    redi[part * FB + fr] = bi;
    __syncthreads();
    if (part == 0 && (MODE == 3 || fr < nf)) {
      for (int k = 1; k < NP; ++k) {
        const double v = red[k * FB + fr];
        const int i = redi[k * FB + fr];
        if (v > best || (v == best && i < bi)) {
          best = v;
          bi = i;
        }
      }
      if (MODE == 2) reinterpret_cast<int64_t *>(out)[f0 + fr] = (bi < M) ? bi + 1 : 1;     // (no log-density above -inf: a NaN frame)
      if (MODE == 3) {
        if (bi >= M) bi = 0;
        redi[fr] = bi;                  // (slot 0 of the frame: written, and read before, by this thread alone)
        if (fr < nf) mhat[f0 + fr] = bi + 1;
      }
    }
    if (MODE == 2) return;
    __syncthreads();
    // phase 3t: prm3 is the trajectory table here, [M][DP][mu_x, a, mu_y, q]; the rows of the tile's padding frames (x = 0,
    // some mixture of the model) and of the padding dimensions (zeros) are computed and never stored
    const double *tp = prm3 + (size_t)redi[fr] * DP * kBdmapPrm4;
#pragma unroll 4
    for (int d = part; d < DP; d += NP) {
      const bdm_d4 r = *reinterpret_cast<const bdm_d4 *>(tp + (size_t)d * kBdmapPrm4);
      xs[d * RS + fr] = r[3] * fma(r[1], xs[d * RS + fr] - r[0], r[2]);
    }
    __syncthreads();
    bdmap_store_tile<FB>(xs, reinterpret_cast<double *>(out), ldy, f0, nf, D, DP);
    return;
  }
  {
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
      L[m * FB + fr] = e;
      s += e;
    }
    red[part * FB + fr] = s;
    __syncthreads();
    s = red[fr];
    for (int k = 1; k < NP; ++k) s += red[k * FB + fr];
    for (int m = part; m < M; m += NP) L[m * FB + fr] = L[m * FB + fr] / s;
  }
  __syncthreads();

  if (MODE == 1) {
    double *P = reinterpret_cast<double *>(out) + f0 * M;       // [T][M]: the workgroup's frames are contiguous
    for (int i = tid; i < nf * M; i += kBdmThreads) {
      const int pf = i / M, m = i - pf * M;
      P[i] = L[m * FB + pf];
    }
    return;
  }

  // phase 3
  for (int dw = 2 * NS * wave; dw < DP; dw += 2 * NS * NW) {
    int db = dw + 2 * sub;
    if (FB == 64) db = __builtin_amdgcn_readfirstlane(db);
    if (db < DP) {
      const double x0 = xs[db * RS + f], x1 = xs[(db + 1) * RS + f];
      double y0 = 0.0, y1 = 0.0;
      const double *pp = prm3 + (size_t)db * kBdmapPrm3;
#pragma unroll 2
      for (int m = 0; m < M; ++m) {
        const double pm = L[m * FB + f];
        const double *t = pp + (size_t)m * DP * kBdmapPrm3;       // [mu_x, a, mu_y, 0] of the two dimensions
        y0 = fma(pm, fma(t[1], x0 - t[0], t[2]), y0);
        y1 = fma(pm, fma(t[5], x1 - t[4], t[6]), y1);
      }
      xs[db * RS + f] = y0;
      xs[(db + 1) * RS + f] = y1;
    }
  }
  __syncthreads();
  bdmap_store_tile<FB>(xs, reinterpret_cast<double *>(out), ldy, f0, nf, D, DP);
}

template <int MODE, int FB>
static int bdmap_launch(const vcmi_bdmap *h, const double *dX, int64_t ldx, int64_t T, void *out, int64_t ldy, hipStream_t st,
                        int64_t *mhat = nullptr) {
  static std::atomic<bool> attr_done[64];
  VCMI_TRY(set_max_dynamic_lds(bdmap_kernel<MODE, FB>, bdmap_lds_bytes(kBdmapMaxD, FB == 64 ? 128 : kBdmapMaxM, FB), attr_done));
  const int64_t nb = (T + FB - 1) / FB;
  hipLaunchKernelGGL((bdmap_kernel<MODE, FB>), dim3((unsigned)nb), dim3(kBdmThreads), bdmap_lds_bytes(h->DP, h->M, FB), st, dX, ldx, T,
                     h->D, h->DP, h->M, h->prm1.p, MODE == 3 ? h->prm4.p : h->prm3.p, h->cst.p, out, ldy, mhat);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// mode 0: out = Y (leading dimension ldy), 1: out = P [T][M], 2: out = int64 indices, 3: out = G (ldy) and the indices to mhat;
// asynchronous on st
static int bdmap_device(const vcmi_bdmap *h, int mode, const double *dX, int64_t ldx, int64_t T, void *out, int64_t ldy,
                        hipStream_t st, int64_t *mhat = nullptr) {
  if (T == 0) return VCMI_OK;
  int dev = 0;
  VCMI_HIP(hipGetDevice(&dev));
  if (dev != h->device)
    return fail(VCMI_ERR_ARG, "vcmi_bdmap: the handle was created on device %d, the call runs on device %d", h->device, dev);
  if ((T + 31) / 32 > 0x7fffffffLL) return fail(VCMI_ERR_DIM, "vcmi_bdmap: %lld frames exceed one launch", (long long)T);
  if (h->FB == 64) {
    if (mode == 0) return bdmap_launch<0, 64>(h, dX, ldx, T, out, ldy, st);
    if (mode == 1) return bdmap_launch<1, 64>(h, dX, ldx, T, out, ldy, st);
    if (mode == 3) return bdmap_launch<3, 64>(h, dX, ldx, T, out, ldy, st, mhat);
    return bdmap_launch<2, 64>(h, dX, ldx, T, out, ldy, st);
  }
  if (mode == 0) return bdmap_launch<0, 32>(h, dX, ldx, T, out, ldy, st);
  if (mode == 1) return bdmap_launch<1, 32>(h, dX, ldx, T, out, ldy, st);
  if (mode == 3) return bdmap_launch<3, 32>(h, dX, ldx, T, out, ldy, st, mhat);
  return bdmap_launch<2, 32>(h, dX, ldx, T, out, ldy, st);
}

static int bdmap_check_xy(const vcmi_bdmap *h, const void *X, int64_t ldx, int64_t T, const void *Y, int64_t ldy, const char *who) {
  if (!h) return fail(VCMI_ERR_ARG, "%s: NULL handle", who);
  if (T < 0) return fail(VCMI_ERR_ARG, "%s: negative frame count", who);
  if (T > 0 && (!X || !Y)) return fail(VCMI_ERR_ARG, "%s: NULL buffer", who);
  if (ldx < h->D) return fail(VCMI_ERR_DIM, "%s: Inconsistent dimensions (leading dimension %lld < dim %d)", who, (long long)ldx, h->D);
  if (ldy < h->D) return fail(VCMI_ERR_DIM, "%s: ldy %lld < dim %d", who, (long long)ldy, h->D);
  return VCMI_OK;
}

int bdmap_traj_device(const vcmi_bdmap *h, const double *dX, int64_t T, int64_t *mhat, double *G, hipStream_t st) {
  return bdmap_device(h, 3, dX, h->D, T, G, h->D, st, mhat);
}

}  // namespace vcmi

using namespace vcmi;

extern "C" int vcmi_bdmap_create(const double *weights, const double *mu, const double *covars, int Dj, int M, int swap,
                                 vcmi_bdmap **out) {
  if (!weights || !mu || !covars || !out) return fail(VCMI_ERR_ARG, "vcmi_bdmap_create: NULL argument");
  *out = nullptr;
  if (Dj < 2 || (Dj & 1) || M < 1)
    return fail(VCMI_ERR_DIM, "vcmi_bdmap_create: joint dimension %d / mixtures %d invalid (the joint dimension must be even)", Dj, M);
  if (Dj / 2 > kBdmapMaxD) return fail(VCMI_ERR_DIM, "vcmi_bdmap_create: dimension %d exceeds the cross-diagonal converter's limit (%d)", Dj / 2, kBdmapMaxD);
  if (M > kBdmapMaxM) return fail(VCMI_ERR_DIM, "vcmi_bdmap_create: %d mixtures exceed the cross-diagonal converter's limit (%d)", M, kBdmapMaxM);
  BdmapTable t;
  const int64_t bad = bdmap_prepare(weights, mu, covars, Dj, M, swap != 0, &t);
  if (bad >= 0) {
    const int D = Dj / 2;
    return fail(VCMI_ERR_NOT_PD, "vcmi_bdmap_create: pair (%d,%d) is not positive definite", (int)(bad % D) + 1, (int)(bad / D) + 1);
  }
  VCMI_TRY(check_device());
  vcmi_bdmap *h = new (std::nothrow) vcmi_bdmap();
  if (!h) return fail(VCMI_ERR_OOM, "out of host memory");
  h->D = t.D;
  h->DP = t.DP;
  h->M = t.M;
  (void)hipGetDevice(&h->device);
  h->FB = bdmap_lds_bytes(t.DP, t.M, 64) <= bdmap_lds_bytes(kBdmapMaxD, 128, 64) ? 64 : 32;
  static_assert(((size_t)128 * 65 + (size_t)128 * 64 + 512) * 8 + 512 * 4 <= kBdmLdsBudget, "the 64-frame tiles fit a CU");
  static_assert(((size_t)128 * 33 + (size_t)256 * 32 + 512) * 8 + 512 * 4 <= kBdmLdsBudget, "the 32-frame tiles fit a CU");
  int rc = upload_now(h->prm1, t.prm1);
  if (rc == VCMI_OK) rc = upload_now(h->prm3, t.prm3);
  if (rc == VCMI_OK) rc = upload_now(h->cst, t.cst);
  if (rc == VCMI_OK) rc = upload_now(h->prm4, t.prm4);
  if (rc != VCMI_OK) {
    delete h;
    return rc;
  }
  h->h_a = std::move(t.a);
  h->h_q = std::move(t.q);
  h->q_bad = t.q_bad;
  *out = h;
  return VCMI_OK;
}

extern "C" int vcmi_bdmap_destroy(vcmi_bdmap *h) {
  delete h;
  return VCMI_OK;
}
extern "C" int vcmi_bdmap_dim(const vcmi_bdmap *h) { return h ? h->D : -1; }
extern "C" int vcmi_bdmap_ncomponents(const vcmi_bdmap *h) { return h ? h->M : -1; }
extern "C" int vcmi_bdmap_get_a(const vcmi_bdmap *h, double *a) {
  if (!h || !a) return fail(VCMI_ERR_ARG, "vcmi_bdmap_get_a: NULL argument");
  memcpy(a, h->h_a.data(), h->h_a.size() * sizeof(double));
  return VCMI_OK;
}

extern "C" int vcmi_bdmap_convert_dev(vcmi_bdmap *h, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy, void *stream) {
  VCMI_TRY(bdmap_check_xy(h, dX, ldx, T, dY, ldy, "vcmi_bdmap_convert_dev"));
  return bdmap_device(h, 0, dX, ldx, T, dY, ldy, as_stream(stream));
}

extern "C" int vcmi_bdmap_convert(vcmi_bdmap *h, const double *X, int64_t ldx, int64_t T, double *Y, int64_t ldy) {
  VCMI_TRY(bdmap_check_xy(h, X, ldx, T, Y, ldy, "vcmi_bdmap_convert"));
  if (T == 0) return VCMI_OK;
  const int D = h->D;
  const size_t row = (size_t)D * 8;
  return staged_pipeline(X, row, (size_t)ldx * 8, Y, row, (size_t)ldy * 8, T, kBdmMinChunkFrames,
                         [&](const void *dIn, void *dOut, int64_t, int64_t n, hipStream_t st) -> int {
                           return bdmap_device(h, 0, (const double *)dIn, D, n, dOut, D, st);
                         });
}

extern "C" int vcmi_bdmap_posterior_dev(vcmi_bdmap *h, const double *dX, int64_t ldx, int64_t T, double *dP, void *stream) {
  VCMI_TRY(bdmap_check_xy(h, dX, ldx, T, dP, h ? h->D : 0, "vcmi_bdmap_posterior_dev"));
  return bdmap_device(h, 1, dX, ldx, T, dP, 0, as_stream(stream));
}

extern "C" int vcmi_bdmap_posterior(vcmi_bdmap *h, const double *X, int64_t ldx, int64_t T, double *P) {
  VCMI_TRY(bdmap_check_xy(h, X, ldx, T, P, h ? h->D : 0, "vcmi_bdmap_posterior"));
  if (T == 0) return VCMI_OK;
  const int D = h->D, M = h->M;
  return staged_pipeline(X, (size_t)D * 8, (size_t)ldx * 8, P, (size_t)M * 8, (size_t)M * 8, T, kBdmMinChunkFrames,
                         [&](const void *dIn, void *dOut, int64_t, int64_t n, hipStream_t st) -> int {
                           return bdmap_device(h, 1, (const double *)dIn, D, n, dOut, 0, st);
                         });
}

extern "C" int vcmi_bdmap_predict_dev(vcmi_bdmap *h, const double *dX, int64_t ldx, int64_t T, int64_t *didx, void *stream) {
  VCMI_TRY(bdmap_check_xy(h, dX, ldx, T, didx, h ? h->D : 0, "vcmi_bdmap_predict_dev"));
  return bdmap_device(h, 2, dX, ldx, T, didx, 0, as_stream(stream));
}

extern "C" int vcmi_bdmap_predict(vcmi_bdmap *h, const double *X, int64_t ldx, int64_t T, int64_t *idx) {
  VCMI_TRY(bdmap_check_xy(h, X, ldx, T, idx, h ? h->D : 0, "vcmi_bdmap_predict"));
  if (T == 0) return VCMI_OK;
  const int D = h->D;
  return staged_pipeline(X, (size_t)D * 8, (size_t)ldx * 8, idx, 8, 8, T, kBdmMinChunkFrames,
                         [&](const void *dIn, void *dOut, int64_t, int64_t n, hipStream_t st) -> int {
                           return bdmap_device(h, 2, (const double *)dIn, D, n, dOut, 0, st);
                         });
}

// vc(c::FrameByFrameConverter, fm), src/common.jl:7-26, with fvpostf!(VarianceScaling(sigma2), converted[2:end, :]) (src/gv.jl:10-15)
// when sigma2 is given: vcmi_vc_frames / vcmi_vc_frames_postf for this converter.  Rows 2..D+1 of the (D+1,T) matrix are
// converted where they lie (leading dimension D + 1).
extern "C" int vcmi_vc_bdmap(vcmi_bdmap *h, const double *fm, int64_t T, const double *sigma2, double *out) {
  if (!h) return fail(VCMI_ERR_ARG, "vcmi_vc_bdmap: NULL handle");
  if (T < 0 || (T > 0 && (!fm || !out))) return fail(VCMI_ERR_ARG, "vcmi_vc_bdmap: bad argument");
  if (T == 0) return VCMI_OK;
  const int D = h->D;
  const int64_t ld = D + 1;          // row 1 is the power coefficient, src/common.jl:11
  const size_t row = (size_t)ld * 8;
  if (!sigma2)
    return staged_pipeline(fm, row, row, out, row, row, T, kBdmMinChunkFrames,
                           [&](const void *dIn, void *dOut, int64_t, int64_t n, hipStream_t st) -> int {
                             // the copy keeps row 1 (src/common.jl:23); the kernel then overwrites rows 2..D+1
                             VCMI_HIP(hipMemcpyAsync(dOut, dIn, (size_t)n * row, hipMemcpyDefault, st));
                             return bdmap_device(h, 0, (const double *)dIn + 1, ld, n, (double *)dOut + 1, ld, st);
                           });
  if (T < 2) return fail(VCMI_ERR_DIM, "vcmi_vc_bdmap: the variance of a one-frame matrix is undefined");
  VCMI_TRY(check_device());
  const size_t bytes = row * (size_t)T;
  VcScratch &sc = vc_scratch();
  VcScratch::Release release{sc};
  VCMI_TRY(sc.stage.reserve((size_t)2 * ld * T));                    // fm, and the result behind it
  double *din = sc.stage.p, *dout = sc.stage.p + (size_t)ld * T;
  VCMI_TRY(staged_upload(din, fm, bytes, nullptr));
  VCMI_HIP(hipMemcpyAsync(dout, din, bytes, hipMemcpyDeviceToDevice, nullptr));
  VCMI_TRY(bdmap_device(h, 0, din + 1, ld, T, dout + 1, ld, nullptr));
  VCMI_TRY(variance_scaling_device(dout + 1, ld, D, T, sigma2, dout + 1, ld, nullptr));
  return staged_download(out, dout, bytes, nullptr);
}

extern "C" int vcmi_vc_bdmap_batch(vcmi_bdmap *h, int64_t n, const double *const *fm, const int64_t *T, const double *sigma2,
                                   double *const *out) {
  if (!h) return fail(VCMI_ERR_ARG, "vcmi_vc_bdmap_batch: NULL handle");
  return vc_frames_batch(h->D, [h](const double *dX, int64_t ld, int64_t N, double *dY, hipStream_t st) -> int {
                           return bdmap_device(h, 0, dX, ld, N, dY, ld, st);
                         }, n, fm, T, sigma2, out, "vcmi_vc_bdmap_batch");
}
