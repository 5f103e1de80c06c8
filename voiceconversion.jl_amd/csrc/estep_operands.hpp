// estep_operands.hpp -- from the model parameters to the operands of the MFMA kernels (included by estep.hip): the pinned
// staging ring of the host-parameter entry points, the copy kernel that takes a slot to the device, and estep_prep_kernel.
#pragma once
#include "estep_cfg.hpp"

namespace vcmi {

// Pinned staging (a ring of slots) for the (tiny) model parameters of the MFMA path: the copy to the device is a real
// asynchronous copy, the host buffers outlive the call, and nothing in the call waits for the GPU -- consecutive
// E-steps queue back to back (the first version packed on the host and drained the stream before every launch:
// 0.4 ms of a 2.3 ms step).
struct EstepStaging {
  // a ring of eight: a caller issuing E-steps back to back blocks on the event of the slot it is about to reuse, and a
  // blocked host thread wakes up late on a busy machine -- with eight calls queued the GPU does not run dry meanwhile
  static constexpr int kSlots = 8;
  double *host[kSlots] = {};
  hipEvent_t copied[kSlots] = {};
  size_t cap = 0;
  int next = 0;
  int reserve(size_t n) {
    if (n <= cap) return VCMI_OK;
    release();
    for (int i = 0; i < kSlots; ++i) {
      VCMI_HIP(hipHostMalloc(reinterpret_cast<void **>(&host[i]), n * sizeof(double), hipHostMallocDefault));
      VCMI_HIP(hipEventCreateWithFlags(&copied[i], hipEventDisableTiming));
    }
    cap = n;
    return VCMI_OK;
  }
  void release() {
    for (int i = 0; i < kSlots; ++i) {
      if (host[i]) (void)hipHostFree(host[i]);
      if (copied[i]) (void)hipEventDestroy(copied[i]);
      host[i] = nullptr;
      copied[i] = nullptr;
    }
    cap = 0;
  }
  ~EstepStaging() { release(); }
};

// model parameters: pinned host slot -> device
__global__ void __launch_bounds__(256) estep_param_copy_kernel(const double *__restrict__ src, double *__restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// raw = [w (M) | mu (DJ,M) | var (DJ,M)] on the device -> the MFMA kernel's operands:
//   Wpack[mt][ks][lane]: A-operand fragments of W[m][k], k < DJ -> -1/(2 var) (multiplies x^2), k >= DJ -> mu/var
//   cinit[m] = log w - (DJ log 2pi + sum log var)/2 - sum mu^2/(2 var)   (-inf for m >= M and for zero weights)
template <int DJ>
__global__ void __launch_bounds__(256)
estep_prep_kernel(const double *__restrict__ raw, int M, int dj, double *__restrict__ Wpack, double *__restrict__ cinit,
                  double *__restrict__ refiv, double *__restrict__ refc) {
  using C = EstepCfg<DJ>;
  const double *w = raw, *mu = raw + M, *var = mu + (size_t)dj * M;      // dj <= DJ: the data's dimension
  const int e = blockIdx.x * 256 + threadIdx.x;
  // operands of the exact re-evaluation (estep_mfma_kernel, "refinement"): 1/var in the parameters' own (dj,M) layout and
  // the constant WITHOUT the -mu^2/(2 var) term
  if (e < M * dj) refiv[e] = 1.0 / var[e];
  if (e < 8 * C::KS * 64) {
    const int l = e & 63, ks = (e >> 6) % C::KS, mt = (e >> 6) / C::KS;
    const int m = 16 * mt + (l & 15), k = 4 * ks + (l >> 4);
    double v = 0.0;
    const int d = k < DJ ? k : k - DJ;
    if (m < M && d < dj) {                      // zero weights for the padding dimensions dj .. DJ-1
      const double ivv = 1.0 / var[d + (size_t)dj * m];
      v = k < DJ ? -0.5 * ivv : mu[d + (size_t)dj * m] * ivv;
    }
    Wpack[e] = v;
  }
  // the constants: sixteen lanes per mixture share the sums over d (log var is the expensive part: one thread per mixture
  // walking all dj dimensions, twice, took 50 us), combined by xor butterflies -- a fixed order, the same in every lane
  if (e < 16 * C::MMAX) {
    const int m = e >> 4, l = e & 15;
    double sl = 0.0, t = 0.0;
    if (m < M)
      for (int d = l; d < dj; d += 16) {
        const double vv = var[d + (size_t)dj * m], mm = mu[d + (size_t)dj * m];
        sl += log(vv);
        t += mm * mm * (1.0 / vv);
      }
#pragma unroll
    for (int sh = 8; sh >= 1; sh >>= 1) {
      sl += __shfl_xor(sl, sh);
      t += __shfl_xor(t, sh);
    }
    if (l == 0) {
      const double base = (m < M) ? (w[m] > 0.0 ? log(w[m]) : -INFINITY) - 0.5 * (dj * kLog2Pi + sl) : -INFINITY;
      if (m < M) {
        refc[2 * m] = base;                 // the constant WITHOUT the -mu^2/(2 var) term (exact re-evaluation)
        // When is the expanded form  l^ = sum_d (a_d x_d^2 + b_d x_d) + cinit  good enough?  Its rounding error is at most
        // (2 dj + 6) u T,  T = sum_d |a_d x_d^2| + |b_d x_d| + |cinit|  (u = 2^-53; the accumulation, the rounded operands, x^2).
        // With A = sum x^2/var, C = sum mu^2/var (`t` above) and q = sum (x - mu)^2/var = 2 (base - l):  sum |a x^2| = A / 2,
        // sum |b x| <= sqrt(A C), sqrt(A) <= sqrt(q) + sqrt(C)  =>  T <= (sqrt(q) + 2 sqrt(C))^2 / 2 + |base| <= q + 4 C + |base|.
        // The error stays below 1e-10 (tests: statistics to 1e-9) when q + 4 C + |base| <= Tmax = 1e-10 / ((2 dj + 6) u), i.e. when
        //   l >= base - (Tmax - 4 C - |base|) / 2   =: the threshold -- above `base` (never reached) for the tight-variance models
        // the re-evaluation exists for, far below any competing value for ordinary ones.
        const double tmax = 1e-10 / ((2.0 * dj + 6.0) * 0x1p-53);
        refc[2 * m + 1] = base > -INFINITY ? base - 0.5 * (tmax - 4.0 * t - fabs(base)) : -INFINITY;
      }
      cinit[m] = (m < M) ? base - 0.5 * t : -INFINITY;
    }
  }
}

}  // namespace vcmi
