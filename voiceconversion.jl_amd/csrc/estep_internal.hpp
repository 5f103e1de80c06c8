// estep_internal.hpp -- what crosses estep.hip (diagonal E-step), estep_full.hip (full-covariance E-step), estep_bdiag.hip
// (cross-diagonal E-step) and gmm_em.hip (device-resident EM states).  Host functions, and two inline helpers that host and
// device code share: the library is built without relocatable device code, so a kernel is launched by a host function of
// the file that defines it.
#pragma once
#include "vcmi_common.hpp"
#include "bdiag_pair.hpp"

struct vcmi_gmmmap;

namespace vcmi {

// ---- estep.hip ----
// stats[e] (+)= the nrows partial rows of plen doubles, summed in a fixed order (estep_reduce_kernel); only_if: a device
// word that switches the launch off when it is 0
void estep_reduce_launch(const double *part, int nrows, int64_t plen, double *stats, hipStream_t st, int accumulate = 1,
                         const int64_t *only_if = nullptr);
// out[0] += the n doubles of v, in a fixed order (estep_sum_kernel)
void estep_sum_launch(const double *v, int64_t n, double *out, hipStream_t st);

// The diagonal E-step of N device-resident frames from a DEVICE parameter block [w (M) | mu (Dj,M) | var (Dj,M)] that the
// caller keeps alive and orders on `st`; its variances are positive (the caller has checked them).  Where the MFMA path
// serves (Dj, M) the parameters never leave the device; the other shapes copy the block down (one stream synchronisation)
// and run from the host copy.
int estep_device_block(const double *dX, int64_t N, int Dj, int M, const double *dparams, double *dstats, hipStream_t st);

// One E-step from device-resident frames and HOST parameters -> packed statistics on the device: estep_device (estep.hip)
// and estep_full_device (estep_full.hip); `cov` is var (Dj,M) or sigma (Dj,Dj,M).
using EstepDeviceFn = int (*)(const double *dX, int64_t N, int Dj, int M, const double *w, const double *mu, const double *cov,
                              double *dstats, hipStream_t st);
// The host-pointer E-step of vcmi_estep_diag / vcmi_estep_full: frames up, `dev` per device (group) member, one all-reduce,
// the plen packed statistics unpacked into S0 (M), S1 (Dj,M), S2 (s2len) and *loglik.
int estep_host(EstepDeviceFn dev, const double *X, int64_t N, int Dj, int M, const double *w, const double *mu, const double *cov,
               int64_t plen, size_t s2len, double *S0, double *S1, double *S2, double *loglik);

// the argument checks every E-step entry shares
int estep_check_dims(int64_t N, int Dj, int M);
// index d + Dj m of the first variance (Dj,M) that is not > 0 (a NaN included), -1: none
int64_t first_bad_variance(const double *var, int Dj, int M);
// vcmi_debug_estep_mfma / vcmi_debug_estep_full_mfma on their counter
int mfma_count_hook(DevBuf<unsigned long long> &count, int enable, int64_t *issued);

// ---- estep_bdiag.hip ----
// The cross-diagonal ("block_diag") model: joint row d couples with row d + D only, D = Dj / 2; per mixture the covariances
// are [var (Dj) | c (D)].  Every even Dj in [2, 256] and M in [1, 256]: estep_bdiag_gamma_kernel holds a 64-frame tile of
// Dj rows in LDS, em_mstep_bdiag_kernel is one thread per pair.
constexpr int kBdiagMaxDj = 256, kBdiagMaxM = 256;
// bdiag_det, bdiag_pair_valid and first_bad_pair: bdiag_pair.hpp (no HIP: the host-only preparation files share them)
// VCMI_ERR_DIM unless Dj is even, 2 <= Dj <= kBdiagMaxDj and 1 <= M <= kBdiagMaxM; the message names the limit
int estep_bdiag_check_dims(const char *who, int Dj, int M);
// The E-step of N device-resident frames from a DEVICE parameter block [w (M) | mu (Dj,M) | covars (Dj + D, M)] that the
// caller keeps alive and orders on `st`; asynchronous, no parameter crosses the host.  *dflag (an int the caller has set to
// INT_MAX) receives the smallest 1 + d + D m of an invalid pair; N == 0 zeroes the statistics and launches nothing.
int estep_bdiag_device_block(const double *dX, int64_t N, int Dj, int M, const double *dparams, int *dflag, double *dstats,
                             hipStream_t st);

// ---- estep_full.hip ----
// statistics of N device-resident frames under the prepared p(x) handle -> dstats (zeroed here); asynchronous on st
int estep_full_core(vcmi_gmmmap *px, const double *dX, int64_t N, int Dj, int M, double *dstats, hipStream_t st);
// *d_flag (gmm_px_prepare_device) -> VCMI_ERR_NOT_PD; synchronises st
int read_pd_flag(const int *d_flag, hipStream_t st);

}  // namespace vcmi
