// dtw_device.hpp -- device functions shared by the DTW kernels of dtw_twokernel.hip (recurrence, generic) and dtw_fused.hip
// (align): the transition cost, the align() post-processing and the epilogue arg-min + backward pass + path output.
#pragma once
#include <hip/hip_runtime.h>

#include "dtw_plan.hpp"

namespace vcmi {

__device__ __forceinline__ double dtw_transition(int j, int i) {   // transition(d, j, i), src/dtw.jl:23-31
  return (i == j + 1) ? 0.0 : ((i == j) ? 1.0 : 2.0);
}

// align() post-processing, src/align.jl:20-32, from the 0-based path in LDS (one workgroup per pair)
__device__ void dtw_align_post(const DtwPair &P, const double *__restrict__ seq, int D, const int32_t *path32, int32_t *owner, int32_t *holes) {
  const int S = P.S, T = P.T, tid = threadIdx.x, nthr = blockDim.x;
  if (!P.newtgt) return;
  for (int i = tid; i < S; i += nthr) owner[i] = -1;
  __syncthreads();
  for (int t = tid; t < T; t += nthr) atomicMax(&owner[path32[t]], t);   // newtgt[:,path] = tgt: later frames win
  __syncthreads();
  for (int64_t e = tid; e < (int64_t)S * D; e += nthr) {
    const int i = (int)(e / D), d = (int)(e % D);
    const int k = owner[i];
    P.newtgt[e] = (k >= 0) ? seq[(size_t)D * k + d] : 0.0;
  }
  __shared__ int nholes;
  if (tid == 0) {                                   // hole = setdiff(path[1]:path[end], path), increasing order
    int n = 0;
    for (int i = path32[0]; i <= path32[T - 1]; ++i)
      if (owner[i] < 0 && i > 0 && i < S - 1) holes[n++] = i;   // 1 < i < S in 1-based terms
    nholes = n;
  }
  __syncthreads();
  // each thread owns feature rows d, d+nthr, ...; a row's holes are filled in increasing i, as the reference does
  for (int d = tid; d < D; d += nthr)
    for (int h = 0; h < nholes; ++h) {
      const int i = holes[h];
      P.newtgt[(size_t)D * i + d] = (P.newtgt[(size_t)D * (i - 1) + d] + P.newtgt[(size_t)D * (i + 1) + d]) / 2.0;
    }
}

// shared epilogue: argmin of the last column, backward pass, path output, align post-processing.
// PACKED: the codes are BITS-bit fields of 32-bit words [t / CPW][row] wherever they live (LDS, or global memory when
// LDSCODES is false); otherwise global codes are one byte per cell at P.codes.
template <bool LDSCODES, int BITS, bool PACKED = false>
__device__ void dtw_finish(const DtwPair &P, const double *__restrict__ seq, int D, int fstep, const double *clast, int32_t *path32, int32_t *owner,
                           int32_t *holes, const uint32_t *codes_lds, int Smax) {
  constexpr int CPW = 32 / BITS;
  const int S = P.S, T = P.T, tid = threadIdx.x, nthr = blockDim.x;
  // indmin of the last column (first minimum wins, src/dtw.jl:137): per-thread scan of a strided slice, wave
  // reduction on (value, index) with shuffles, then thread 0 combines the per-wave winners through LDS
  {
    double bv = INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < S; i += nthr) {
      const double c = clast[i];
      if (c < bv) { bv = c; bi = i; }                 // strided, increasing i: keeps the first minimum of the slice
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
      const double ov = __shfl_xor(bv, sh);
      const int oi = __shfl_xor(bi, sh);
      if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    __shared__ double wv_[16];
    __shared__ int wi_[16];
    if ((tid & 63) == 0) { wv_[tid >> 6] = bv; wi_[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
      const int nw = (nthr + 63) >> 6;
      for (int w = 1; w < nw; ++w)
        if (wv_[w] < bv || (wv_[w] == bv && wi_[w] < bi)) { bv = wv_[w]; bi = wi_[w]; }
      int row = bi;
      path32[T - 1] = row;
      for (int t = T - 1; t >= 1; --t) {              // src/dtw.jl:140-142; `row` stays in a register
        int code;
        if (LDSCODES || PACKED) code = (codes_lds[(size_t)(t / CPW) * Smax + row] >> (BITS * (t % CPW))) & ((1u << BITS) - 1u);
        else code = P.codes[(size_t)S * t + row];
        row -= code - fstep;
        path32[t - 1] = row;
      }
    }
  }
  __syncthreads();
  if (P.path)
    for (int t = tid; t < T; t += nthr) P.path[t] = (int64_t)path32[t] + 1;
  dtw_align_post(P, seq, D, path32, owner, holes);
}

}  // namespace vcmi
