// gmm_em.hip -- EM states resident on the device, MI355X (gfx950): vcmi_gmm_em_* (full covariance), vcmi_gmm_em_diag_* and
// vcmi_gmm_em_bdiag_* (cross-diagonal).
//
// bin/train_gmm.jl:84-103 (sklearn.mixture.GMM(covariance_type="full", min_covar).fit): parameters, statistics and
// whitening blocks stay in HBM; one iteration is
//   estep (local statistics) -> [caller all-reduces the statistics buffer over RCCL] -> mstep (+ whitening prep).
// The E-steps are those of estep_full.hip, estep.hip and estep_bdiag.hip (estep_internal.hpp); the M-step kernels are here,
// and open with one helper (mstep_weight).
// Two kinds of state.  vcmi_gmm_em (full covariance) has one parameter block, a p(x) handle and a flag that the whitening
// preparation reads.  vcmi_gmm_em_diag and vcmi_gmm_em_bdiag are two opaque names of ONE two-block state (Em2State): create,
// the M-step's host side (launch, the 16-byte read of {latch, report, loglik}, the latch, the swap of the blocks), get and the
// guard in front of the E-step are written once (em2_*), and a type supplies an Em2Kind -- its dimension check, host validity
// scan, third-parameter length, control words, M-step kernel, E-step call and the unit its report names.
#include "estep_internal.hpp"
#include "gmmmap_handle.hpp"
#include "hostpipe.hpp"

namespace vcmi {

// The opening of the three M-step kernels, called by every thread of the 256-thread workgroup of mixture m: the total of S0
// over M in a fixed order (256 strided partial sums in `red`, an 8-level tree -- no floating-point atomics), then
// *inv = 1 / (S0[m] + 10 eps) and the return value, the weight S0[m] / (total + 10 eps) + eps.  Sums and quotients only:
// nothing here that a compiler could contract, inside or outside an `fp contract(off)` scope.
__device__ inline double mstep_weight(const double *__restrict__ stats, int M, int m, double *red, double *inv) {
  const int tid = threadIdx.x;
  const double eps = 2.220446049250313e-16;
  double t = 0.0;
  for (int k = tid; k < M; k += 256) t += stats[k];
  red[tid] = t;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const double tot = red[0], s0 = stats[m];
  *inv = 1.0 / (s0 + 10 * eps);
  return s0 / (tot + 10 * eps) + eps;
}

__global__ void __launch_bounds__(256)
em_mstep_full_kernel(const double *__restrict__ stats, int Dj, int M, double min_covar, double *__restrict__ w,
                     double *__restrict__ mu, double *__restrict__ sigma, const int *__restrict__ flag) {
  __shared__ double red[256];
  __shared__ double mus[256];
  const int tid = threadIdx.x, m = blockIdx.x;
  // a covariance of the CURRENT parameters was reported not positive definite: the statistics computed under them are NaN
  // for every mixture.  Keep the parameters, so that the preparation that follows reports the same mixture again (and not
  // the last one of a model that is NaN throughout) and vcmi_gmm_em_get still shows the model that failed.
  if (*flag) return;
  double inv;
  const double wm = mstep_weight(stats, M, m, red, &inv);
  const double *S1 = stats + M + (size_t)m * Dj;
  const double *S2 = stats + M + (size_t)M * Dj + (size_t)m * Dj * Dj;
  for (int d = tid; d < Dj; d += 256) {
    const double v = S1[d] * inv;
    mus[d] = v;
    mu[(size_t)m * Dj + d] = v;
  }
  if (tid == 0) w[m] = wm;
  __syncthreads();
  for (int e = tid; e < Dj * Dj; e += 256) {
    const int c = e / Dj, r = e - c * Dj;
    sigma[(size_t)m * Dj * Dj + e] = S2[e] * inv - mus[r] * mus[c] + (r == c ? min_covar : 0.0);
  }
}

// The diagonal twin (estep.py:mstep_diag, operation for operation; the old sklearn GMM's covariance_type="diag" update):
//   stats = [S0 (M) | S1 (Dj,M) | S2 (Dj,M) | loglik]  ->  raw = [w (M) | mu (Dj,M) | var (Dj,M)], the block the diagonal E-step's
//   prep kernels read (estep_prep_kernel, estep_hard_prep_kernel).
// One workgroup per mixture, thread d owns dimension d (Dj <= 256); the total over M in the fixed order of em_mstep_full_kernel
// (256 strided partial sums, a tree): no floating-point atomics, the same statistics give the same bits.  The five roundings of
// the variance are the five of the numpy expression -- no contraction into FMAs.  A variance that is not > 0 (a NaN included)
// is reported through ctl: ctl[1] receives the smallest 1 + d + Dj m (an integer minimum: the same answer whatever the order
// of the workgroups).  ctl[0] is the latch of an EARLIER failed M-step: the kernel then leaves `raw` alone.  ctl[2..3] carry the
// log-likelihood of the statistics, so that the host reads it and the report in one copy.
__global__ void __launch_bounds__(256)
em_mstep_diag_kernel(const double *__restrict__ stats, int Dj, int M, double min_covar, double *__restrict__ raw, int *__restrict__ ctl) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int tid = threadIdx.x, m = blockIdx.x;
  if (m == 0 && tid == 0) *reinterpret_cast<double *>(ctl + 2) = stats[(size_t)M * (1 + 2 * (size_t)Dj)];
  if (ctl[0]) return;
  double inv;
  const double wm = mstep_weight(stats, M, m, red, &inv);
  if (tid == 0) raw[m] = wm;
  if (tid < Dj) {
    const size_t e = (size_t)m * Dj + tid;
    const double s1 = stats[M + e], s2 = stats[M + (size_t)M * Dj + e];
    const double mean = s1 * inv;
    const double v = s2 * inv - ((2.0 * mean) * s1) * inv + mean * mean + min_covar;
    raw[M + e] = mean;
    raw[M + (size_t)M * Dj + e] = v;
    if (!(v > 0.0)) atomicMin(ctl + 1, (int)(1 + e));
  }
}

// The cross-diagonal twin (estep.py:mstep_bdiag, operation for operation):
//   stats = [S0 (M) | S1 (Dj,M) | S2 (Dj,M) | Sxy (D,M) | loglik]  ->  raw = [w (M) | mu (Dj,M) | covars (Dj + D, M)], the block
//   estep_bdiag_prep_kernel reads; covars[:, m] = [var (Dj) | c (D)], c = Sxy inv - mu_d mu_{d+D} (min_covar on variances only).
// One workgroup per mixture, thread d owns PAIR d (D <= 128): both means, both variances and the cross-covariance; the total
// over M, the roundings of the variance and the control block as em_mstep_diag_kernel.  A pair that is not positive definite
// (bdiag_pair_valid; a NaN included) is reported through ctl[1] as the smallest 1 + d + D m.
__global__ void __launch_bounds__(256)
em_mstep_bdiag_kernel(const double *__restrict__ stats, int Dj, int M, double min_covar, double *__restrict__ raw, int *__restrict__ ctl) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int tid = threadIdx.x, m = blockIdx.x, D = Dj / 2;
  if (m == 0 && tid == 0) *reinterpret_cast<double *>(ctl + 2) = stats[(size_t)M * (1 + 2 * (size_t)Dj + D)];
  if (ctl[0]) return;
  double inv;
  const double wm = mstep_weight(stats, M, m, red, &inv);
  if (tid == 0) raw[m] = wm;
  if (tid < D) {
    const double *S1 = stats + M + (size_t)m * Dj, *S2 = stats + M + (size_t)M * Dj + (size_t)m * Dj;
    const double sxy = stats[M + 2 * (size_t)M * Dj + (size_t)m * D + tid];
    double mean[2], v[2];
    for (int h = 0; h < 2; ++h) {
      const double s1 = S1[tid + h * D], s2 = S2[tid + h * D];
      mean[h] = s1 * inv;
      v[h] = s2 * inv - ((2.0 * mean[h]) * s1) * inv + mean[h] * mean[h] + min_covar;
    }
    const double c = sxy * inv - mean[0] * mean[1];
    double *mu = raw + M + (size_t)m * Dj, *cv = raw + M + (size_t)M * Dj + (size_t)m * (Dj + D);
    mu[tid] = mean[0];
    mu[tid + D] = mean[1];
    cv[tid] = v[0];
    cv[tid + D] = v[1];
    cv[tid + Dj] = c;
    if (!bdiag_pair_valid(v[0], v[1], c)) atomicMin(ctl + 1, 1 + tid + D * m);
  }
}

}  // namespace vcmi

struct vcmi_gmm_em {
  int Dj = 0, M = 0, device = 0;
  double min_covar = 0.0;
  bool prepared = false;
  vcmi::DevBuf<double> params;   // [w (M) | mu (Dj,M) | sigma (Dj,Dj,M)]
  vcmi::DevBuf<int> flag;
  vcmi_gmmmap *px = nullptr;
  ~vcmi_gmm_em() { delete px; }
  double *w() { return params.p; }
  double *mu() { return params.p + M; }
  double *sigma() { return params.p + M + (size_t)M * Dj; }
  int64_t plen() const { return (int64_t)M * (1 + Dj + (int64_t)Dj * Dj) + 1; }
};

namespace vcmi {
static int em_prepare(vcmi_gmm_em *h, hipStream_t st) {
  // a host preparation that fails (not positive definite) deletes the handle: the state is unprepared until one succeeds,
  // so that the next E-step prepares (and reports) again instead of running on a handle that is gone
  h->prepared = false;
  if (gmm_px_device_prepare_supported(h->Dj)) {
    VCMI_TRY(gmm_px_prepare_device(&h->px, h->w(), h->mu(), h->sigma(), h->Dj, h->M, h->flag.p, st));
  } else {
    // dimensions without a device preparation (198 < Dj <= 256: px_prep_kernel serves Dj <= 99, px_prep_packed_kernel
    // 100 <= Dj <= 198 -- and 99 < Dj whose padded size has an MFMA instantiation; there is none today): Cholesky on the
    // host, with a stream synchronisation
    const size_t dd = (size_t)h->Dj * h->Dj;
    std::vector<double> hw(h->M), hmu((size_t)h->M * h->Dj), hs((size_t)h->M * dd);
    VCMI_HIP(hipStreamSynchronize(st));
    VCMI_HIP(hipMemcpy(hw.data(), h->w(), hw.size() * 8, hipMemcpyDeviceToHost));
    VCMI_HIP(hipMemcpy(hmu.data(), h->mu(), hmu.size() * 8, hipMemcpyDeviceToHost));
    VCMI_HIP(hipMemcpy(hs.data(), h->sigma(), hs.size() * 8, hipMemcpyDeviceToHost));
    VCMI_TRY(gmm_px_create(hw.data(), hmu.data(), hs.data(), h->Dj, h->M, &h->px));
  }
  h->prepared = true;
  return VCMI_OK;
}
}  // namespace vcmi

// ---- the two-block state: diagonal and cross-diagonal -----------------------------------------------
// `raw` holds TWO parameter blocks [w | mu (Dj,M) | third], third = var (Dj,M) or covars (Dj + D, M): the E-step reads block
// `cur`, the M-step kernel writes the other one, and em2_mstep -- which synchronises anyway -- makes that one current only when
// nothing was reported.  So a failed M-step leaves the parameters its statistics were computed under, whichever workgroup
// found the variance or pair and whichever had already written.
namespace vcmi {

// What a covariance type supplies.  A report counts in `units` per mixture (dimensions or pairs): index u + units m.
struct Em2Kind {
  int (*check_dims)(const char *who, int Dj, int M);
  int64_t (*first_bad)(const double *third, int Dj, int M);   // the host validity scan: index of the first bad unit, -1: none
  int (*third_len)(int Dj);                                   // doubles of the third parameter per mixture
  int (*units)(int Dj);
  int (*not_valid)(const char *who, int u, int m);            // VCMI_ERR_NOT_PD naming unit (u, m), 1-based
  int nctl;   // control words: [latch | smallest bad 1 + index (INT_MAX: none) | loglik (a double)], then the E-step's own
  void (*mstep_kernel)(const double *stats, int Dj, int M, double min_covar, double *raw, int *ctl);
  int (*estep)(const double *dX, int64_t N, int Dj, int M, const double *dparams, int *ctl, double *dstats, hipStream_t st);
};

struct Em2State {
  const Em2Kind *kind = nullptr;
  int Dj = 0, M = 0, device = 0, cur = 0;
  double min_covar = 0.0;
  bool failed = false;           // an M-step reported a unit: the state takes no further E-step
  int bad = 0;                   // ... 1 + u + units m of that unit
  DevBuf<double> raw;            // 2 x nraw()
  DevBuf<int> ctl;               // kind->nctl words
  size_t nthird() const { return (size_t)M * kind->third_len(Dj); }
  size_t nraw() const { return (size_t)M * (1 + (size_t)Dj) + nthird(); }
  double *params() { return raw.p + (size_t)cur * nraw(); }
  double *next() { return raw.p + (size_t)(1 - cur) * nraw(); }
  int not_pd() const {
    const int U = kind->units(Dj);
    return kind->not_valid("M-step", (bad - 1) % U + 1, (bad - 1) / U + 1);
  }
};

// H: the opaque handle type of the entry, an Em2State and nothing more
template <class H>
static int em2_create(const Em2Kind &k, const char *who, int Dj, int M, const double *w, const double *mu, const double *third,
                      double min_covar, H **out) {
  if (!w || !mu || !third || !out) return fail(VCMI_ERR_ARG, "%s: NULL argument", who);
  *out = nullptr;
  VCMI_TRY(k.check_dims(who, Dj, M));
  if (!(min_covar >= 0.0)) return fail(VCMI_ERR_ARG, "%s: min_covar must be >= 0", who);
  const int64_t bad = k.first_bad(third, Dj, M);
  if (bad >= 0) return k.not_valid(who, (int)(bad % k.units(Dj)) + 1, (int)(bad / k.units(Dj)) + 1);
  VCMI_TRY(check_device());
  H *h = new (std::nothrow) H();
  if (!h) return fail(VCMI_ERR_OOM, "out of host memory");
  h->kind = &k;
  h->Dj = Dj;
  h->M = M;
  h->min_covar = min_covar;
  (void)hipGetDevice(&h->device);
  int rc = h->raw.alloc(2 * h->nraw());
  if (rc == VCMI_OK) rc = h->ctl.alloc(k.nctl);
  if (rc != VCMI_OK) {
    delete h;
    return rc;
  }
  const int ctl0[6] = {0, INT32_MAX, 0, 0, INT32_MAX, 0};      // (word 4: the report of the cross-diagonal E-step's preparation)
  const size_t md = (size_t)M * Dj;
  hipError_t e = upload_now_hip(h->raw.p, w, sizeof(double) * M);
  if (e == hipSuccess) e = upload_now_hip(h->raw.p + M, mu, sizeof(double) * md);
  if (e == hipSuccess) e = upload_now_hip(h->raw.p + M + md, third, sizeof(double) * h->nthird());
  if (e == hipSuccess) e = upload_now_hip(h->ctl.p, ctl0, sizeof(int) * k.nctl);
  if (e != hipSuccess) {
    delete h;
    return fail(VCMI_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  }
  *out = h;
  return VCMI_OK;
}

static int em2_estep(Em2State *h, const char *who, const double *dX, int64_t N, double *dstats, void *stream) {
  if (!h || !dstats) return fail(VCMI_ERR_ARG, "%s: NULL argument", who);
  if (N < 0 || (N > 0 && !dX)) return fail(VCMI_ERR_ARG, "%s: bad frame block", who);
  if (h->failed) return h->not_pd();
  // (every unit of the block is valid: create and every M-step since have checked them)
  return h->kind->estep(dX, N, h->Dj, h->M, h->params(), h->ctl.p, dstats, as_stream(stream));
}

static int em2_mstep(Em2State *h, const char *who, const double *dstats, void *stream, double *loglik) {
  if (!h || !dstats) return fail(VCMI_ERR_ARG, "%s: NULL argument", who);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(h->kind->mstep_kernel, dim3(h->M), dim3(256), 0, st, dstats, h->Dj, h->M, h->min_covar, h->next(), h->ctl.p);
  VCMI_HIP(hipGetLastError());
  struct {
    int latch, bad;
    double ll;
  } r = {0, 0, 0.0};
  static_assert(sizeof(r) == 16, "the control block starts with two ints and a double");
  VCMI_HIP(hipMemcpyAsync(&r, h->ctl.p, sizeof(r), hipMemcpyDeviceToHost, st));
  VCMI_HIP(hipStreamSynchronize(st));
  if (loglik) *loglik = r.ll;
  if (r.bad != INT32_MAX) {
    if (!h->failed) {      // latch it on the device too: a later M-step kernel returns before it writes
      const int one = 1;
      VCMI_HIP(hipMemcpy(h->ctl.p, &one, sizeof(int), hipMemcpyHostToDevice));
    }
    h->failed = true;
    h->bad = r.bad;
    return h->not_pd();
  }
  h->cur = 1 - h->cur;
  return VCMI_OK;
}

static int em2_get(Em2State *h, const char *who, double *w, double *mu, double *third) {
  if (!h || !w || !mu || !third) return fail(VCMI_ERR_ARG, "%s: NULL argument", who);
  VCMI_HIP(hipDeviceSynchronize());
  const size_t md = (size_t)h->M * h->Dj;
  VCMI_HIP(hipMemcpy(w, h->params(), sizeof(double) * h->M, hipMemcpyDeviceToHost));
  VCMI_HIP(hipMemcpy(mu, h->params() + h->M, sizeof(double) * md, hipMemcpyDeviceToHost));
  VCMI_HIP(hipMemcpy(third, h->params() + h->M + md, sizeof(double) * h->nthird(), hipMemcpyDeviceToHost));
  return VCMI_OK;
}

static int em_diag_check_dims(const char *who, int Dj, int M) {
  if (Dj < 1 || M < 1) return fail(VCMI_ERR_DIM, "%s: Dj=%d M=%d invalid", who, Dj, M);
  if (Dj > 256)   // em_mstep_diag_kernel: one thread of a 256-thread workgroup per dimension
    return fail(VCMI_ERR_DIM, "%s: joint dimension %d exceeds the device EM limit (256)", who, Dj);
  if ((int64_t)M * Dj >= INT32_MAX) return fail(VCMI_ERR_DIM, "%s: Dj=%d M=%d too large", who, Dj, M);
  return VCMI_OK;
}

// the diagonal state: units are dimensions, four control words
static const Em2Kind kEmDiag = {
    em_diag_check_dims,
    first_bad_variance,
    [](int Dj) { return Dj; },
    [](int Dj) { return Dj; },
    [](const char *who, int d, int m) { return fail(VCMI_ERR_NOT_PD, "%s: variance (%d,%d) is not positive", who, d, m); },
    4,
    em_mstep_diag_kernel,
    [](const double *dX, int64_t N, int Dj, int M, const double *dparams, int *, double *dstats, hipStream_t st) {
      return estep_device_block(dX, N, Dj, M, dparams, dstats, st);
    }};

// the cross-diagonal state: units are pairs, two more control words for the E-step preparation's report (ctl + 4, INT_MAX: none)
static const Em2Kind kEmBdiag = {
    estep_bdiag_check_dims,
    first_bad_pair,
    [](int Dj) { return Dj + Dj / 2; },
    [](int Dj) { return Dj / 2; },
    [](const char *who, int d, int m) { return fail(VCMI_ERR_NOT_PD, "%s: pair (%d,%d) is not positive definite", who, d, m); },
    6,
    em_mstep_bdiag_kernel,
    [](const double *dX, int64_t N, int Dj, int M, const double *dparams, int *ctl, double *dstats, hipStream_t st) {
      return estep_bdiag_device_block(dX, N, Dj, M, dparams, ctl + 4, dstats, st);
    }};

}  // namespace vcmi

// two distinct opaque types, one state
struct vcmi_gmm_em_diag : vcmi::Em2State {};
struct vcmi_gmm_em_bdiag : vcmi::Em2State {};

using namespace vcmi;

// ---- device-resident EM state --------------------------------------------------------------------
extern "C" int vcmi_gmm_em_create(int Dj, int M, const double *w, const double *mu, const double *sigma, double min_covar,
                                  vcmi_gmm_em **out) {
  if (!w || !mu || !sigma || !out) return fail(VCMI_ERR_ARG, "vcmi_gmm_em_create: NULL argument");
  *out = nullptr;
  if (Dj < 1 || M < 1) return fail(VCMI_ERR_DIM, "vcmi_gmm_em_create: Dj=%d M=%d invalid", Dj, M);
  if (Dj > 256)   // em_mstep_full_kernel stages the mean vector in a 256-entry LDS array
    return fail(VCMI_ERR_DIM, "vcmi_gmm_em_create: joint dimension %d exceeds the device EM limit (256)", Dj);
  if (!(min_covar >= 0.0)) return fail(VCMI_ERR_ARG, "vcmi_gmm_em_create: min_covar must be >= 0");
  VCMI_TRY(check_device());
  vcmi_gmm_em *h = new (std::nothrow) vcmi_gmm_em();
  if (!h) return fail(VCMI_ERR_OOM, "out of host memory");
  h->Dj = Dj;
  h->M = M;
  h->min_covar = min_covar;
  (void)hipGetDevice(&h->device);
  const size_t dd = (size_t)Dj * Dj;
  int rc = h->params.alloc((size_t)M * (1 + Dj + dd));
  if (rc == VCMI_OK) rc = h->flag.alloc(1);
  if (rc != VCMI_OK) {
    delete h;
    return rc;
  }
  hipError_t e = upload_now_hip(h->w(), w, sizeof(double) * M);
  if (e == hipSuccess) e = upload_now_hip(h->mu(), mu, sizeof(double) * M * Dj);
  if (e == hipSuccess) e = upload_now_hip(h->sigma(), sigma, sizeof(double) * M * dd);
  if (e == hipSuccess) e = hipMemset(h->flag.p, 0, sizeof(int));
  if (e != hipSuccess) {
    delete h;
    return fail(VCMI_ERR_HIP, "vcmi_gmm_em_create: %s", hipGetErrorString(e));
  }
  *out = h;
  return VCMI_OK;
}

extern "C" int vcmi_gmm_em_destroy(vcmi_gmm_em *h) {
  delete h;
  return VCMI_OK;
}

extern "C" int vcmi_gmm_em_estep_dev(vcmi_gmm_em *h, const double *dX, int64_t N, double *dstats, void *stream) {
  if (!h || !dstats) return fail(VCMI_ERR_ARG, "vcmi_gmm_em_estep_dev: NULL argument");
  if (N < 0 || (N > 0 && !dX)) return fail(VCMI_ERR_ARG, "vcmi_gmm_em_estep_dev: bad frame block");
  hipStream_t st = as_stream(stream);
  if (!h->prepared) VCMI_TRY(em_prepare(h, st));
  return estep_full_core(h->px, dX, N, h->Dj, h->M, dstats, st);
}

extern "C" int vcmi_gmm_em_mstep(vcmi_gmm_em *h, const double *dstats, void *stream, double *loglik) {
  if (!h || !dstats) return fail(VCMI_ERR_ARG, "vcmi_gmm_em_mstep: NULL argument");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(em_mstep_full_kernel, dim3(h->M), dim3(256), 0, st, dstats, h->Dj, h->M, h->min_covar, h->w(), h->mu(),
                     h->sigma(), h->flag.p);
  VCMI_HIP(hipGetLastError());
  VCMI_TRY(em_prepare(h, st));
  double ll = 0.0;
  VCMI_HIP(hipMemcpyAsync(&ll, dstats + (h->plen() - 1), sizeof(double), hipMemcpyDeviceToHost, st));
  VCMI_TRY(read_pd_flag(h->flag.p, st));   // synchronises: covers the initial and the new parameters
  if (loglik) *loglik = ll;
  return VCMI_OK;
}

extern "C" int vcmi_gmm_em_get(vcmi_gmm_em *h, double *w, double *mu, double *sigma) {
  if (!h || !w || !mu || !sigma) return fail(VCMI_ERR_ARG, "vcmi_gmm_em_get: NULL argument");
  VCMI_HIP(hipDeviceSynchronize());
  const size_t dd = (size_t)h->Dj * h->Dj;
  VCMI_HIP(hipMemcpy(w, h->w(), sizeof(double) * h->M, hipMemcpyDeviceToHost));
  VCMI_HIP(hipMemcpy(mu, h->mu(), sizeof(double) * h->M * h->Dj, hipMemcpyDeviceToHost));
  VCMI_HIP(hipMemcpy(sigma, h->sigma(), sizeof(double) * h->M * dd, hipMemcpyDeviceToHost));
  return VCMI_OK;
}

// ---- device-resident diagonal EM state -----------------------------------------------------------
extern "C" int vcmi_gmm_em_diag_create(int Dj, int M, const double *w, const double *mu, const double *var, double min_covar,
                                       vcmi_gmm_em_diag **out) {
  return em2_create(kEmDiag, "vcmi_gmm_em_diag_create", Dj, M, w, mu, var, min_covar, out);
}

extern "C" int vcmi_gmm_em_diag_destroy(vcmi_gmm_em_diag *h) {
  delete h;
  return VCMI_OK;
}

extern "C" int vcmi_gmm_em_diag_estep_dev(vcmi_gmm_em_diag *h, const double *dX, int64_t N, double *dstats, void *stream) {
  return em2_estep(h, "vcmi_gmm_em_diag_estep_dev", dX, N, dstats, stream);
}

extern "C" int vcmi_gmm_em_diag_mstep(vcmi_gmm_em_diag *h, const double *dstats, void *stream, double *loglik) {
  return em2_mstep(h, "vcmi_gmm_em_diag_mstep", dstats, stream, loglik);
}

extern "C" int vcmi_gmm_em_diag_get(vcmi_gmm_em_diag *h, double *w, double *mu, double *var) {
  return em2_get(h, "vcmi_gmm_em_diag_get", w, mu, var);
}

// ---- device-resident cross-diagonal EM state -----------------------------------------------------
extern "C" int vcmi_gmm_em_bdiag_create(int Dj, int M, const double *w, const double *mu, const double *covars, double min_covar,
                                        vcmi_gmm_em_bdiag **out) {
  return em2_create(kEmBdiag, "vcmi_gmm_em_bdiag_create", Dj, M, w, mu, covars, min_covar, out);
}

extern "C" int vcmi_gmm_em_bdiag_destroy(vcmi_gmm_em_bdiag *h) {
  delete h;
  return VCMI_OK;
}

extern "C" int vcmi_gmm_em_bdiag_estep_dev(vcmi_gmm_em_bdiag *h, const double *dX, int64_t N, double *dstats, void *stream) {
  return em2_estep(h, "vcmi_gmm_em_bdiag_estep_dev", dX, N, dstats, stream);
}

extern "C" int vcmi_gmm_em_bdiag_mstep(vcmi_gmm_em_bdiag *h, const double *dstats, void *stream, double *loglik) {
  return em2_mstep(h, "vcmi_gmm_em_bdiag_mstep", dstats, stream, loglik);
}

extern "C" int vcmi_gmm_em_bdiag_get(vcmi_gmm_em_bdiag *h, double *w, double *mu, double *covars) {
  return em2_get(h, "vcmi_gmm_em_bdiag_get", w, mu, covars);
}
