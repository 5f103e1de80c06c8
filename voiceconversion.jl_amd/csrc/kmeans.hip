// kmeans.hip -- device k-means (sklearn 0.17 KMeans semantics) over a (Dj,N) column-major block of frames: the
// initialisation that sklearn.mixture.GMM(init_params="wmc") runs over ALL of X before the EM loop (bin/train_gmm.jl:84-89).
//
// Kernels
//  * km_assign_kernel<KS> (Dj <= 160; the hot path): nearest center and its squared distance for every frame.  The cross
//    term x.c runs on v_mfma_f64_16x16x4_f64 (centers = A, 16 per tile; frames = B, 16 per wave; k = 4 dimensions per
//    step, Dj zero-padded to 4 KS, which changes no distance).  The expanded form e = |x|^2 - 2 x.c + |c|^2 is only a
//    screen: with bnd = (6 Dj + 24) 2^-53 (|x| + |c|)^2, which covers the rounding of e and of the direct difference,
//    every center whose e - bnd is not above the running bound U (min over e + bnd and over the direct values found so
//    far) is re-evaluated as sum_d (x_d - c_d)^2 in FP64, sequentially in d, without contraction (km_direct).  The
//    winner is the smallest direct value, exact ties to the smaller index: labels and distances are those of the direct
//    difference whatever the cancellation in e (data far from the origin just sends more centers to the direct path).
//  * km_assign_direct_kernel (Dj > 160): one thread per frame, every center by direct difference.
//  * km_stats_kernel: per-cluster statistics as a one-hot GEMM on the same MFMA, rows [x (Dj) | 1 | mind2] times
//    onehot(label): P frame chunks, each summed in frame order into its own partial; km_stats_reduce_kernel adds the
//    partials in chunk order and km_inertia_kernel adds the per-cluster distance sums in cluster order.  No atomics on
//    floating-point data: identical inputs give identical bits.
//  * update (centers = sum x / count, summed squared shift), relocation of empty clusters (the e-th empty cluster takes
//    the frame with the e-th largest mind2, ties to the smaller frame index; top-E by E rounds of an arg-max that
//    excludes the keys already taken), greedy k-means++ (sklearn _k_init: potentials of the L local trials in one pass,
//    inclusive prefix of mind2 over 256-frame segments for the searchsorted of the host's u * potential).
#include "vcmi_common.hpp"

#include <cmath>
#include <limits>

using vcmi::DevBuf;
using vcmi::fail;

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int KM_SEG = 256;          // frames per potential segment (one block of the seeding kernels)
constexpr int KM_MAX_TRIALS = 16;    // local trials of one seeding step (2 + floor(ln 1024) = 8 at the largest M)
constexpr int KM_MFMA_MAX_DJ = 160;

// sum_d (x_d - c_d)^2, sequential in d, each operation rounded on its own: the reference value of every distance.  The file
// is built with -ffp-contract=off (Makefile): the helpers below are plain operators, which hipcc would otherwise fuse.
__device__ __forceinline__ double km_direct(const double *__restrict__ x, const double *__restrict__ c, int Dj) {
  double s = 0.0;
  for (int d = 0; d < Dj; ++d) {
    const double t = __dsub_rn(x[d], c[d]);
    s = __dadd_rn(s, __dmul_rn(t, t));
  }
  return s;
}

__device__ __forceinline__ bool km_better(double d, int m, double bd, int bm) { return d < bd || (d == bd && m < bm); }

// centers (Dj,M) -> MFMA A fragments in lane order (tile t, k-step ks, lane l holds c[4 ks + l/16, 16 t + l%16]; zero
// padding), |c|^2 and |c| per center
__global__ void __launch_bounds__(256) km_prep_kernel(const double *__restrict__ C, int Dj, int M, int KS, int MT,
                                                       double *__restrict__ frag, double *__restrict__ cn,
                                                       double *__restrict__ cs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nfrag = (int64_t)MT * KS * 64;
  if (i < nfrag) {
    const int lane = (int)(i & 63);
    const int ks = (int)((i >> 6) % KS);
    const int t = (int)(i / (64 * (int64_t)KS));
    const int m = t * 16 + (lane & 15), d = ks * 4 + (lane >> 4);
    frag[i] = (m < M && d < Dj) ? C[d + (int64_t)m * Dj] : 0.0;
  }
  if (i < M) {
    double s = 0.0;
    for (int d = 0; d < Dj; ++d) s += C[d + i * Dj] * C[d + i * Dj];
    cn[i] = s;
    cs[i] = sqrt(s);
  }
}

__device__ __forceinline__ void km_flag_nonfinite(double v, int *flag) {
  if (!isfinite(v)) atomicOr(flag, 1);   // integer flag: read once by the host, order-independent
}

// One wave = 16 frames; block = 4 waves.  Lane l: frame n0 + (l & 15); the accumulator holds centers 16 t + (l >> 4) + 4 r.
template <int KS>
__global__ void __launch_bounds__(256) km_assign_kernel(const double *__restrict__ X, int64_t N, int Dj, int M, int MT,
                                                         const double *__restrict__ C, const double *__restrict__ frag,
                                                         const double *__restrict__ cn, const double *__restrict__ cs,
                                                         int *__restrict__ labels, int *__restrict__ labels_out,
                                                         double *__restrict__ mind2, int *__restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t n0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (n0 >= N) return;   // whole wave out of range (no barriers in this kernel)
  const int j = lane & 15, kk = lane >> 4;
  const int64_t f = n0 + j;
  const bool fv = f < N;
  const double *xf = X + (fv ? f : n0) * (int64_t)Dj;
  double xb[KS];
  double xx = 0.0;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int d = ks * 4 + kk;
    xb[ks] = (fv && d < Dj) ? xf[d] : 0.0;
    xx += xb[ks] * xb[ks];
  }
  xx += __shfl_xor(xx, 16);
  xx += __shfl_xor(xx, 32);
  if (fv && kk == 0) km_flag_nonfinite(xx, flag);
  const double xs = sqrt(xx);
  const double kb = (6.0 * Dj + 24.0) * 0x1p-53;
  double U = INFINITY, bd = INFINITY;
  int bm = 0x7fffffff;
  for (int t = 0; t < MT; ++t) {
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    const double *ft = frag + (int64_t)t * KS * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ft[ks * 64], xb[ks], acc, 0, 0, 0);
    double e[4], b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = t * 16 + kk + 4 * r;
      if (m < M) {
        e[r] = xx + cn[m] - 2.0 * acc[r];
        const double s = xs + cs[m];
        b[r] = kb * s * s;
        U = fmin(U, e[r] + b[r]);
      } else {
        e[r] = INFINITY;
        b[r] = 0.0;
      }
    }
    U = fmin(U, __shfl_xor(U, 16));
    U = fmin(U, __shfl_xor(U, 32));
    if (fv) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = t * 16 + kk + 4 * r;
        if (m < M && !(e[r] - b[r] > U)) {    // (a NaN screen value also takes the direct path)
          const double d = km_direct(xf, C + (int64_t)m * Dj, Dj);
          if (km_better(d, m, bd, bm)) {
            bd = d;
            bm = m;
          }
          U = fmin(U, d);
        }
      }
    }
    U = fmin(U, __shfl_xor(U, 16));
    U = fmin(U, __shfl_xor(U, 32));
  }
  // combine the four lane groups of each frame (same frame, disjoint center subsets)
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const double od = __shfl_xor(bd, o);
    const int om = __shfl_xor(bm, o);
    if (km_better(od, om, bd, bm)) {
      bd = od;
      bm = om;
    }
  }
  if (fv && kk == 0) {
    if (bm >= M) {   // NaN input: no center compares; keep the label in range, the flag reports the frame
      bm = 0;
      atomicOr(flag, 1);
    }
    labels[f] = bm;
    if (labels_out) labels_out[f] = bm;
    mind2[f] = bd;
  }
}

__global__ void __launch_bounds__(256) km_assign_direct_kernel(const double *__restrict__ X, int64_t N, int Dj, int M,
                                                                const double *__restrict__ C, int *__restrict__ labels,
                                                                int *__restrict__ labels_out, double *__restrict__ mind2,
                                                                int *__restrict__ flag) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= N) return;
  const double *xf = X + f * Dj;
  double bd = INFINITY;
  int bm = 0x7fffffff;
  for (int m = 0; m < M; ++m) {
    const double d = km_direct(xf, C + (int64_t)m * Dj, Dj);
    if (km_better(d, m, bd, bm)) {
      bd = d;
      bm = m;
    }
  }
  if (bm >= M || !isfinite(bd)) {
    atomicOr(flag, 1);
    if (bm >= M) bm = 0;
  }
  labels[f] = bm;
  if (labels_out) labels_out[f] = bm;
  mind2[f] = bd;
}

// Partial statistics of frame chunk p = blockIdx.x: part[p][row][m] = sum over the chunk's frames (in order) of
// row(x) * [label == m], rows [x_0 .. x_{Dj-1}, 1, mind2].  A = 16 rows x 4 frames, B = 4 frames x 16 clusters (one-hot).
__global__ void __launch_bounds__(256) km_stats_kernel(const double *__restrict__ X, int64_t N, int Dj, int Mp, int64_t L,
                                                        const int *__restrict__ labels, const double *__restrict__ mind2,
                                                        double *__restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int m0 = (blockIdx.z * 4 + (threadIdx.x >> 6)) * 16;
  if (m0 >= Mp) return;
  const int R = Dj + 2;
  const int r0 = blockIdx.y * 16;
  const int64_t p = blockIdx.x;
  const int64_t lo = p * L, hi = lo + L < N ? lo + L : N;
  const int i = lane & 15, k = lane >> 4;
  const int row = r0 + i;
  const int mj = m0 + (lane & 15);
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int64_t f0 = lo; f0 < hi; f0 += 4) {
    const int64_t f = f0 + k;
    double a = 0.0, bv = 0.0;
    if (f < hi) {
      a = row < Dj ? X[f * Dj + row] : row == Dj ? 1.0 : row == Dj + 1 ? mind2[f] : 0.0;
      bv = labels[f] == mj ? 1.0 : 0.0;
    }
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc, 0, 0, 0);
  }
  double *out = part + p * (int64_t)R * Mp;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int orow = r0 + (lane >> 4) + 4 * r;
    if (orow < R) out[(int64_t)orow * Mp + mj] = acc[r];
  }
}

// stats = [count (M) | sum x (Dj,M) | inertia]; clsd (M) = per-cluster distance sums (summed by km_inertia_kernel)
__global__ void __launch_bounds__(256) km_stats_reduce_kernel(const double *__restrict__ part, int64_t P, int Dj, int M,
                                                               int Mp, double *__restrict__ stats, double *__restrict__ clsd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int R = Dj + 2;
  if (i >= (int64_t)R * M) return;
  const int row = (int)(i / M), m = (int)(i % M);
  double s = 0.0;
  for (int64_t p = 0; p < P; ++p) s += part[(p * R + row) * Mp + m];
  if (row < Dj) stats[M + row + (int64_t)m * Dj] = s;
  else if (row == Dj) stats[m] = s;
  else clsd[m] = s;
}

__global__ void km_inertia_kernel(const double *__restrict__ clsd, int M, int Dj, double *__restrict__ stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int m = 0; m < M; ++m) s += clsd[m];
  stats[M + (int64_t)Dj * M] = s;
}

// centers <- sum x / count for every non-empty cluster (an empty one keeps its center until km_relocate); prev <- old
__global__ void __launch_bounds__(256) km_update_kernel(const double *__restrict__ stats, int Dj, int M,
                                                         double *__restrict__ C, double *__restrict__ prev,
                                                         int *__restrict__ n_empty, int *__restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)Dj * M) return;
  const int m = (int)(i / Dj), d = (int)(i % Dj);
  const double cnt = stats[m];
  const double old = C[i];
  prev[i] = old;
  if (cnt > 0.0) {
    const double v = stats[M + i] / cnt;
    km_flag_nonfinite(v, flag);
    C[i] = v;
  } else if (d == 0) {
    atomicAdd(n_empty, 1);   // integer count
  }
}

// scal[0] = sum (C - prev)^2 in a fixed order (one block)
__global__ void __launch_bounds__(256) km_shift_kernel(const double *__restrict__ C, const double *__restrict__ prev,
                                                        int64_t n, double *__restrict__ scal) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double t = C[i] - prev[i];
    s += t * t;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) scal[0] = red[0];
}

// Top-E of (mind2 descending, frame index ascending), one key per round: the largest key strictly below `prevkey`.
struct KmKey {
  double v;
  int64_t i;
};
__device__ __forceinline__ bool km_key_gt(double v, int64_t i, double bv, int64_t bi) {
  return v > bv || (v == bv && i < bi);
}

__global__ void __launch_bounds__(256) km_far_partial_kernel(const double *__restrict__ mind2, int64_t N,
                                                              const KmKey *__restrict__ prevkey, KmKey *__restrict__ part) {
  __shared__ double sv[256];
  __shared__ int64_t si[256];
  const double pv = prevkey->v;
  const int64_t pi = prevkey->i;
  double bv = -INFINITY;
  int64_t bi = -1;
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < N; f += (int64_t)gridDim.x * 256) {
    const double v = mind2[f];
    if (km_key_gt(pv, pi, v, f) && (bi < 0 || km_key_gt(v, f, bv, bi))) {
      bv = v;
      bi = f;
    }
  }
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const double v = sv[threadIdx.x + o];
      const int64_t i = si[threadIdx.x + o];
      if (i >= 0 && (si[threadIdx.x] < 0 || km_key_gt(v, i, sv[threadIdx.x], si[threadIdx.x]))) {
        sv[threadIdx.x] = v;
        si[threadIdx.x] = i;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = KmKey{sv[0], si[0]};
}

// reduce the partials in block order; record r = [mind2, global index (or -1), x (Dj)]; prevkey <- the pick
__global__ void __launch_bounds__(256) km_far_final_kernel(const KmKey *__restrict__ part, int G, const double *__restrict__ X,
                                                            int Dj, int64_t offset, KmKey *__restrict__ prevkey,
                                                            double *__restrict__ rec) {
  __shared__ KmKey best;
  if (threadIdx.x == 0) {
    KmKey b{-INFINITY, -1};
    for (int g = 0; g < G; ++g)
      if (part[g].i >= 0 && (b.i < 0 || km_key_gt(part[g].v, part[g].i, b.v, b.i))) b = part[g];
    best = b;
    rec[0] = b.i >= 0 ? b.v : -INFINITY;
    rec[1] = b.i >= 0 ? (double)(b.i + offset) : -1.0;
    if (b.i >= 0) *prevkey = b;
  }
  __syncthreads();
  for (int d = threadIdx.x; d < Dj; d += blockDim.x) rec[2 + d] = best.i >= 0 ? X[best.i * Dj + d] : 0.0;
}

// the e-th empty cluster (ascending index) takes the e-th best candidate record (mind2 descending, global index ascending)
__global__ void __launch_bounds__(256) km_relocate_kernel(const double *__restrict__ stats, int Dj, int M,
                                                           const double *__restrict__ cand, int64_t ncand,
                                                           double *__restrict__ C, int *__restrict__ taken) {
  __shared__ int64_t pick;
  __shared__ int cid;
  if (threadIdx.x == 0) {
    for (int64_t c = 0; c < ncand; ++c) taken[c] = 0;
    cid = -1;
  }
  __syncthreads();
  for (;;) {
    if (threadIdx.x == 0) {
      int m = cid + 1;
      while (m < M && stats[m] > 0.0) ++m;
      cid = m;
      pick = -1;
      if (m < M) {
        for (int64_t c = 0; c < ncand; ++c) {
          const double *r = cand + c * (Dj + 2);
          if (taken[c] || r[1] < 0.0) continue;
          if (pick < 0) { pick = c; continue; }
          const double *b = cand + pick * (Dj + 2);
          if (r[0] > b[0] || (r[0] == b[0] && r[1] < b[1])) pick = c;
        }
        if (pick >= 0) taken[pick] = 1;
      }
    }
    __syncthreads();
    if (cid >= M || pick < 0) break;
    for (int d = threadIdx.x; d < Dj; d += blockDim.x) C[d + (int64_t)cid * Dj] = cand[pick * (Dj + 2) + 2 + d];
    __syncthreads();
  }
}

// ---------------------------------------------------------------- seeding
// mind2 <- min(mind2, |x - c|^2) (reset: |x - c|^2); segsum[s] = fixed-order tree sum of the segment's mind2
__global__ void __launch_bounds__(KM_SEG) km_seed_commit_kernel(const double *__restrict__ X, int64_t N, int Dj,
                                                                 const double *__restrict__ c, int reset,
                                                                 double *__restrict__ mind2, double *__restrict__ segsum,
                                                                 int *__restrict__ flag) {
  __shared__ double red[KM_SEG];
  const int64_t f = (int64_t)blockIdx.x * KM_SEG + threadIdx.x;
  double v = 0.0;
  if (f < N) {
    const double d = km_direct(X + f * Dj, c, Dj);
    km_flag_nonfinite(d, flag);
    v = reset ? d : fmin(mind2[f], d);
    mind2[f] = v;
  }
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = KM_SEG / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) segsum[blockIdx.x] = red[0];
}

// potential of L trial centers cand (Dj,L): segment partials, same tree as km_seed_commit_kernel
__global__ void __launch_bounds__(KM_SEG) km_seed_trials_kernel(const double *__restrict__ X, int64_t N, int Dj,
                                                                 const double *__restrict__ cand, int L,
                                                                 const double *__restrict__ mind2, int64_t nseg,
                                                                 double *__restrict__ segpot) {
  __shared__ double red[KM_SEG];
  const int64_t f = (int64_t)blockIdx.x * KM_SEG + threadIdx.x;
  for (int l = 0; l < L; ++l) {
    red[threadIdx.x] = f < N ? fmin(mind2[f], km_direct(X + f * Dj, cand + (int64_t)l * Dj, Dj)) : 0.0;
    __syncthreads();
    for (int o = KM_SEG / 2; o > 0; o >>= 1) {
      if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) segpot[l * nseg + blockIdx.x] = red[0];
    __syncthreads();
  }
}

// out[l] = sum over segments (in order) of seg[l * nseg + s]; one thread per row
__global__ void km_seg_total_kernel(const double *__restrict__ seg, int64_t nseg, int L, double *__restrict__ out) {
  const int l = threadIdx.x;
  if (l >= L) return;
  double s = 0.0;
  for (int64_t i = 0; i < nseg; ++i) s += seg[l * nseg + i];
  out[l] = s;
}

// idx[l] = first frame whose inclusive prefix of mind2 (segment totals in order, then the frames of the segment in order)
// reaches t[l]; N - 1 when none does (sklearn clips the same way)
__global__ void km_seed_pick_kernel(const double *__restrict__ mind2, int64_t N, const double *__restrict__ segsum,
                                    int64_t nseg, const double *__restrict__ t, int L, int64_t *__restrict__ idx) {
  const int l = threadIdx.x;
  if (l >= L) return;
  const double tl = t[l];
  double c = 0.0;
  int64_t s = 0;
  for (; s < nseg; ++s) {
    if (c + segsum[s] >= tl) break;
    c += segsum[s];
  }
  int64_t r = N - 1;
  if (s < nseg) {
    const int64_t lo = s * KM_SEG, hi = lo + KM_SEG < N ? lo + KM_SEG : N;
    r = hi - 1;
    for (int64_t f = lo; f < hi; ++f) {
      c += mind2[f];
      if (c >= tl) {
        r = f;
        break;
      }
    }
  }
  idx[l] = r;
}

template <int KS>
void launch_assign(dim3 g, hipStream_t st, const double *X, int64_t N, int Dj, int M, int MT, const double *C,
                   const double *frag, const double *cn, const double *cs, int *lab, int *lab_out, double *mind2, int *flag) {
  hipLaunchKernelGGL(km_assign_kernel<KS>, g, dim3(256), 0, st, X, N, Dj, M, MT, C, frag, cn, cs, lab, lab_out, mind2, flag);
}

}  // namespace

struct vcmi_kmeans {
  int Dj = 0, M = 0, KS = 0, MT = 0, Mp = 0;
  DevBuf<double> C, prev, best, frag, cn, cs;
  DevBuf<double> mind2, part, clsd, segsum, segpot, scal, cand, targets, rec;
  DevBuf<int> labels, flag, taken;
  DevBuf<int64_t> pick;
  DevBuf<KmKey> farpart, prevkey;
  int64_t nlast = -1;          // frames of the last assignment / seeding pass (mind2, labels refer to them)
  double best_inertia = INFINITY;
  double pending_inertia = 0.0;
  bool prepared = false;
};

namespace {

int km_ks_for(int Dj) {
  const int ks = (Dj + 3) / 4;
  static const int buckets[] = {2, 4, 8, 12, 16, 20, 24, 32, 40};
  for (int b : buckets)
    if (ks <= b) return b;
  return 0;   // Dj > 160: direct kernel
}

int km_prepare(vcmi_kmeans *h, hipStream_t st) {
  if (h->prepared) return VCMI_OK;
  const int64_t nfrag = (int64_t)h->MT * (h->KS ? h->KS : 1) * 64;
  const int64_t n = nfrag > h->M ? nfrag : h->M;
  hipLaunchKernelGGL(km_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->C.p, h->Dj, h->M,
                     h->KS ? h->KS : 1, h->MT, h->frag.p, h->cn.p, h->cs.p);
  VCMI_HIP(hipGetLastError());
  h->prepared = true;
  return VCMI_OK;
}

int km_frames(vcmi_kmeans *h, int64_t N) {
  if (N <= (int64_t)h->mind2.n && N <= (int64_t)h->labels.n) return VCMI_OK;
  VCMI_TRY(h->mind2.reserve((size_t)N));
  VCMI_TRY(h->labels.reserve((size_t)N));
  return VCMI_OK;
}

int km_read_flag(vcmi_kmeans *h, hipStream_t st, const char *who) {
  int f = 0;
  VCMI_HIP(hipMemcpyAsync(&f, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  VCMI_HIP(hipStreamSynchronize(st));
  if (f) {
    VCMI_HIP(hipMemsetAsync(h->flag.p, 0, sizeof(int), st));
    VCMI_HIP(hipStreamSynchronize(st));
    return fail(VCMI_ERR_ARG, "%s: non-finite frame or center value", who);
  }
  return VCMI_OK;
}

// after the centers are final for this iteration: shift, best-center tracking
int km_finish_update(vcmi_kmeans *h, hipStream_t st, double *shift) {
  hipLaunchKernelGGL(km_shift_kernel, dim3(1), dim3(256), 0, st, h->C.p, h->prev.p, (int64_t)h->Dj * h->M, h->scal.p);
  VCMI_HIP(hipGetLastError());
  double s = 0.0;
  VCMI_HIP(hipMemcpyAsync(&s, h->scal.p, sizeof(double), hipMemcpyDeviceToHost, st));
  if (h->pending_inertia < h->best_inertia) {
    h->best_inertia = h->pending_inertia;
    VCMI_HIP(hipMemcpyAsync(h->best.p, h->C.p, sizeof(double) * h->Dj * h->M, hipMemcpyDeviceToDevice, st));
  }
  VCMI_HIP(hipStreamSynchronize(st));
  h->prepared = false;
  if (shift) *shift = s;
  return VCMI_OK;
}

bool host_finite(const double *v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

}  // namespace

extern "C" int64_t vcmi_kmeans_stats_len(int Dj, int M) {
  if (Dj < 1 || M < 1) return 0;
  return (int64_t)M * (1 + Dj) + 1;
}

extern "C" int vcmi_kmeans_create(int Dj, int M, const double *centers0, vcmi_kmeans **out) {
  if (!out) return fail(VCMI_ERR_ARG, "vcmi_kmeans_create: NULL argument");
  *out = nullptr;
  if (Dj < 1 || Dj > 256 || M < 1 || M > 1024)
    return fail(VCMI_ERR_DIM, "vcmi_kmeans_create: Dj=%d M=%d outside 1..256 x 1..1024", Dj, M);
  if (centers0 && !host_finite(centers0, (size_t)Dj * M))
    return fail(VCMI_ERR_ARG, "vcmi_kmeans_create: non-finite initial center");
  VCMI_TRY(vcmi::check_device());
  vcmi_kmeans *h = new (std::nothrow) vcmi_kmeans();
  if (!h) return fail(VCMI_ERR_OOM, "out of host memory");
  h->Dj = Dj;
  h->M = M;
  h->KS = Dj <= KM_MFMA_MAX_DJ ? km_ks_for(Dj) : 0;
  h->MT = (M + 15) / 16;
  h->Mp = h->MT * 16;
  const size_t dm = (size_t)Dj * M;
  int rc = VCMI_OK;
  for (DevBuf<double> *b : {&h->C, &h->prev, &h->best}) if (rc == VCMI_OK) rc = b->alloc(dm);
  if (rc == VCMI_OK) rc = h->frag.alloc((size_t)h->MT * (h->KS ? h->KS : 1) * 64);
  if (rc == VCMI_OK) rc = h->cn.alloc(M);
  if (rc == VCMI_OK) rc = h->cs.alloc(M);
  if (rc == VCMI_OK) rc = h->clsd.alloc(M);
  if (rc == VCMI_OK) rc = h->scal.alloc(4);
  if (rc == VCMI_OK) rc = h->flag.alloc(1);
  if (rc == VCMI_OK) rc = h->prevkey.alloc(1);
  if (rc == VCMI_OK) rc = h->pick.alloc(KM_MAX_TRIALS);
  if (rc == VCMI_OK) rc = h->targets.alloc(KM_MAX_TRIALS);
  if (rc != VCMI_OK) {
    delete h;
    return rc;
  }
  hipError_t e = centers0 ? hipMemcpy(h->C.p, centers0, sizeof(double) * dm, hipMemcpyHostToDevice)
                          : hipMemset(h->C.p, 0, sizeof(double) * dm);
  if (e == hipSuccess) e = hipMemcpy(h->best.p, h->C.p, sizeof(double) * dm, hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipMemset(h->flag.p, 0, sizeof(int));
  if (e != hipSuccess) {
    delete h;
    return fail(VCMI_ERR_HIP, "vcmi_kmeans_create: %s", hipGetErrorString(e));
  }
  *out = h;
  return VCMI_OK;
}

extern "C" int vcmi_kmeans_destroy(vcmi_kmeans *h) {
  delete h;
  return VCMI_OK;
}

extern "C" int vcmi_kmeans_set(vcmi_kmeans *h, const double *centers) {
  if (!h || !centers) return fail(VCMI_ERR_ARG, "vcmi_kmeans_set: NULL argument");
  if (!host_finite(centers, (size_t)h->Dj * h->M)) return fail(VCMI_ERR_ARG, "vcmi_kmeans_set: non-finite center");
  VCMI_HIP(hipDeviceSynchronize());
  VCMI_HIP(hipMemcpy(h->C.p, centers, sizeof(double) * h->Dj * h->M, hipMemcpyHostToDevice));
  h->prepared = false;
  return VCMI_OK;
}

extern "C" int vcmi_kmeans_get(vcmi_kmeans *h, double *centers) {
  if (!h || !centers) return fail(VCMI_ERR_ARG, "vcmi_kmeans_get: NULL argument");
  VCMI_HIP(hipDeviceSynchronize());
  VCMI_HIP(hipMemcpy(centers, h->C.p, sizeof(double) * h->Dj * h->M, hipMemcpyDeviceToHost));
  return VCMI_OK;
}

extern "C" int vcmi_kmeans_restore_best(vcmi_kmeans *h) {
  if (!h) return fail(VCMI_ERR_ARG, "vcmi_kmeans_restore_best: NULL argument");
  VCMI_HIP(hipDeviceSynchronize());
  if (std::isfinite(h->best_inertia))
    VCMI_HIP(hipMemcpy(h->C.p, h->best.p, sizeof(double) * h->Dj * h->M, hipMemcpyDeviceToDevice));
  h->prepared = false;
  return VCMI_OK;
}

extern "C" int vcmi_kmeans_assign_dev(vcmi_kmeans *h, const double *dX, int64_t N, double *dstats, int *dlabels,
                                      void *stream) {
  if (!h || !dstats) return fail(VCMI_ERR_ARG, "vcmi_kmeans_assign_dev: NULL argument");
  if (N < 0 || (N > 0 && !dX)) return fail(VCMI_ERR_ARG, "vcmi_kmeans_assign_dev: bad frame block");
  hipStream_t st = vcmi::as_stream(stream);
  const int Dj = h->Dj, M = h->M, R = Dj + 2;
  VCMI_TRY(km_frames(h, N));
  VCMI_TRY(km_prepare(h, st));
  h->nlast = N;
  if (N == 0) {
    VCMI_HIP(hipMemsetAsync(dstats, 0, sizeof(double) * vcmi_kmeans_stats_len(Dj, M), st));
    return VCMI_OK;
  }
  if (h->KS) {
    const dim3 g((unsigned)((N + 63) / 64));
    switch (h->KS) {
#define KM_CASE(K) \
  case K: launch_assign<K>(g, st, dX, N, Dj, M, h->MT, h->C.p, h->frag.p, h->cn.p, h->cs.p, h->labels.p, dlabels, h->mind2.p, h->flag.p); break;
      KM_CASE(2) KM_CASE(4) KM_CASE(8) KM_CASE(12) KM_CASE(16) KM_CASE(20) KM_CASE(24) KM_CASE(32) KM_CASE(40)
#undef KM_CASE
      default: return fail(VCMI_ERR_ARG, "vcmi_kmeans_assign_dev: no kernel for Dj=%d", Dj);
    }
  } else {
    hipLaunchKernelGGL(km_assign_direct_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, dX, N, Dj, M, h->C.p,
                       h->labels.p, dlabels, h->mind2.p, h->flag.p);
  }
  VCMI_HIP(hipGetLastError());
  // statistics: P chunks of L frames (L a multiple of 4); partials bounded to 2^24 doubles
  const int64_t per = (int64_t)R * h->Mp;
  int64_t P = (N + 2047) / 2048;
  const int64_t Pmax = ((int64_t)1 << 24) / per > 1 ? ((int64_t)1 << 24) / per : 1;
  if (P > Pmax) P = Pmax;
  if (P > 65535) P = 65535;
  int64_t L = (N + P - 1) / P;
  L = (L + 3) / 4 * 4;
  P = (N + L - 1) / L;
  VCMI_TRY(h->part.reserve((size_t)(P * per)));
  const dim3 gs((unsigned)P, (unsigned)((R + 15) / 16), (unsigned)((h->Mp + 63) / 64));
  hipLaunchKernelGGL(km_stats_kernel, gs, dim3(256), 0, st, dX, N, Dj, h->Mp, L, h->labels.p, h->mind2.p, h->part.p);
  VCMI_HIP(hipGetLastError());
  hipLaunchKernelGGL(km_stats_reduce_kernel, dim3((unsigned)(((int64_t)R * M + 255) / 256)), dim3(256), 0, st, h->part.p, P,
                     Dj, M, h->Mp, dstats, h->clsd.p);
  VCMI_HIP(hipGetLastError());
  hipLaunchKernelGGL(km_inertia_kernel, dim3(1), dim3(64), 0, st, h->clsd.p, M, Dj, dstats);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

extern "C" int vcmi_kmeans_update(vcmi_kmeans *h, const double *dstats, void *stream, double *shift, double *inertia,
                                  int *n_empty) {
  if (!h || !dstats) return fail(VCMI_ERR_ARG, "vcmi_kmeans_update: NULL argument");
  hipStream_t st = vcmi::as_stream(stream);
  const int Dj = h->Dj, M = h->M;
  int *ne = reinterpret_cast<int *>(h->scal.p + 1);   // scal[1] holds the integer count of empty clusters
  VCMI_HIP(hipMemsetAsync(ne, 0, sizeof(int), st));
  hipLaunchKernelGGL(km_update_kernel, dim3((unsigned)(((int64_t)Dj * M + 255) / 256)), dim3(256), 0, st, dstats, Dj, M,
                     h->C.p, h->prev.p, ne, h->flag.p);
  VCMI_HIP(hipGetLastError());
  double in = 0.0;
  int e = 0;
  VCMI_HIP(hipMemcpyAsync(&in, dstats + vcmi_kmeans_stats_len(Dj, M) - 1, sizeof(double), hipMemcpyDeviceToHost, st));
  VCMI_HIP(hipMemcpyAsync(&e, ne, sizeof(int), hipMemcpyDeviceToHost, st));
  VCMI_TRY(km_read_flag(h, st, "vcmi_kmeans_update"));
  if (!std::isfinite(in)) return fail(VCMI_ERR_ARG, "vcmi_kmeans_update: non-finite inertia");
  h->pending_inertia = in;
  h->prepared = false;
  if (inertia) *inertia = in;
  if (n_empty) *n_empty = e;
  if (e == 0) return km_finish_update(h, st, shift);
  if (shift) *shift = NAN;   // known after vcmi_kmeans_relocate
  return VCMI_OK;
}

extern "C" int vcmi_kmeans_far_dev(vcmi_kmeans *h, const double *dX, int64_t N, int E, int64_t offset, double *drec,
                                   void *stream) {
  if (!h || !drec || E < 1 || E > h->M) return fail(VCMI_ERR_ARG, "vcmi_kmeans_far_dev: bad argument");
  if (N != h->nlast || (N > 0 && !dX)) return fail(VCMI_ERR_ARG, "vcmi_kmeans_far_dev: X is not the block of the last assignment");
  hipStream_t st = vcmi::as_stream(stream);
  const int G = N > 0 ? (int)((N + 255) / 256 < 1024 ? (N + 255) / 256 : 1024) : 1;
  VCMI_TRY(h->farpart.reserve(G));
  const KmKey start{INFINITY, -1};
  VCMI_HIP(hipMemcpyAsync(h->prevkey.p, &start, sizeof(KmKey), hipMemcpyHostToDevice, st));
  for (int r = 0; r < E; ++r) {
    hipLaunchKernelGGL(km_far_partial_kernel, dim3(G), dim3(256), 0, st, h->mind2.p, N, h->prevkey.p, h->farpart.p);
    hipLaunchKernelGGL(km_far_final_kernel, dim3(1), dim3(256), 0, st, h->farpart.p, G, dX, h->Dj, offset, h->prevkey.p,
                       drec + (int64_t)r * (h->Dj + 2));
  }
  VCMI_HIP(hipGetLastError());
  VCMI_HIP(hipStreamSynchronize(st));   // `start` lives on this stack frame
  return VCMI_OK;
}

extern "C" int vcmi_kmeans_relocate(vcmi_kmeans *h, const double *dstats, const double *dcand, int64_t ncand, void *stream,
                                    double *shift) {
  if (!h || !dstats || (ncand > 0 && !dcand) || ncand < 0) return fail(VCMI_ERR_ARG, "vcmi_kmeans_relocate: bad argument");
  hipStream_t st = vcmi::as_stream(stream);
  VCMI_TRY(h->taken.reserve(ncand > 0 ? ncand : 1));
  hipLaunchKernelGGL(km_relocate_kernel, dim3(1), dim3(256), 0, st, dstats, h->Dj, h->M, dcand, ncand, h->C.p, h->taken.p);
  VCMI_HIP(hipGetLastError());
  return km_finish_update(h, st, shift);
}

extern "C" int vcmi_kmeans_seed_commit(vcmi_kmeans *h, const double *dX, int64_t N, int c, const double *dcenter,
                                       void *stream, double *potential) {
  if (!h || !dcenter || !potential || c < 0 || c >= h->M) return fail(VCMI_ERR_ARG, "vcmi_kmeans_seed_commit: bad argument");
  if (N < 0 || (N > 0 && !dX)) return fail(VCMI_ERR_ARG, "vcmi_kmeans_seed_commit: bad frame block");
  if (c > 0 && N != h->nlast) return fail(VCMI_ERR_ARG, "vcmi_kmeans_seed_commit: X is not the block seeding started on");
  hipStream_t st = vcmi::as_stream(stream);
  const int Dj = h->Dj;
  VCMI_TRY(km_frames(h, N));
  const int64_t nseg = (N + KM_SEG - 1) / KM_SEG;
  VCMI_TRY(h->segsum.reserve(nseg > 0 ? nseg : 1));
  VCMI_HIP(hipMemcpyAsync(h->C.p + (int64_t)c * Dj, dcenter, sizeof(double) * Dj, hipMemcpyDeviceToDevice, st));
  h->prepared = false;
  h->nlast = N;
  if (N > 0) {
    hipLaunchKernelGGL(km_seed_commit_kernel, dim3((unsigned)nseg), dim3(KM_SEG), 0, st, dX, N, Dj, h->C.p + (int64_t)c * Dj,
                       c == 0 ? 1 : 0, h->mind2.p, h->segsum.p, h->flag.p);
    hipLaunchKernelGGL(km_seg_total_kernel, dim3(1), dim3(64), 0, st, h->segsum.p, nseg, 1, h->scal.p + 2);
    VCMI_HIP(hipGetLastError());
  } else {
    VCMI_HIP(hipMemsetAsync(h->scal.p + 2, 0, sizeof(double), st));
  }
  double pot = 0.0;
  VCMI_HIP(hipMemcpyAsync(&pot, h->scal.p + 2, sizeof(double), hipMemcpyDeviceToHost, st));
  VCMI_TRY(km_read_flag(h, st, "vcmi_kmeans_seed_commit"));
  *potential = pot;
  return VCMI_OK;
}

extern "C" int vcmi_kmeans_seed_pick(vcmi_kmeans *h, int L, const double *targets, void *stream, int64_t *idx) {
  if (!h || !targets || !idx || L < 1 || L > KM_MAX_TRIALS) return fail(VCMI_ERR_ARG, "vcmi_kmeans_seed_pick: bad argument");
  if (h->nlast < 1) return fail(VCMI_ERR_ARG, "vcmi_kmeans_seed_pick: no frames committed on this handle");
  hipStream_t st = vcmi::as_stream(stream);
  const int64_t nseg = (h->nlast + KM_SEG - 1) / KM_SEG;
  VCMI_HIP(hipMemcpyAsync(h->targets.p, targets, sizeof(double) * L, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(km_seed_pick_kernel, dim3(1), dim3(64), 0, st, h->mind2.p, h->nlast, h->segsum.p, nseg, h->targets.p, L,
                     h->pick.p);
  VCMI_HIP(hipGetLastError());
  VCMI_HIP(hipMemcpyAsync(idx, h->pick.p, sizeof(int64_t) * L, hipMemcpyDeviceToHost, st));
  VCMI_HIP(hipStreamSynchronize(st));
  return VCMI_OK;
}

extern "C" int vcmi_kmeans_seed_trials(vcmi_kmeans *h, const double *dX, int64_t N, const double *dcand, int L, void *stream,
                                       double *potentials) {
  if (!h || !dcand || !potentials || L < 1 || L > KM_MAX_TRIALS)
    return fail(VCMI_ERR_ARG, "vcmi_kmeans_seed_trials: bad argument");
  if (N != h->nlast || (N > 0 && !dX)) return fail(VCMI_ERR_ARG, "vcmi_kmeans_seed_trials: X is not the block seeding started on");
  hipStream_t st = vcmi::as_stream(stream);
  if (N == 0) {
    for (int l = 0; l < L; ++l) potentials[l] = 0.0;
    return VCMI_OK;
  }
  const int64_t nseg = (N + KM_SEG - 1) / KM_SEG;
  VCMI_TRY(h->segpot.reserve((size_t)(nseg * L)));
  VCMI_TRY(h->rec.reserve(KM_MAX_TRIALS));
  hipLaunchKernelGGL(km_seed_trials_kernel, dim3((unsigned)nseg), dim3(KM_SEG), 0, st, dX, N, h->Dj, dcand, L, h->mind2.p, nseg,
                     h->segpot.p);
  hipLaunchKernelGGL(km_seg_total_kernel, dim3(1), dim3(64), 0, st, h->segpot.p, nseg, L, h->rec.p);
  VCMI_HIP(hipGetLastError());
  VCMI_HIP(hipMemcpyAsync(potentials, h->rec.p, sizeof(double) * L, hipMemcpyDeviceToHost, st));
  VCMI_HIP(hipStreamSynchronize(st));
  return VCMI_OK;
}

extern "C" int vcmi_kmeans_mind2_dev(vcmi_kmeans *h, int64_t N, double *dmind2, void *stream) {
  if (!h || !dmind2 || N != h->nlast || N < 0) return fail(VCMI_ERR_ARG, "vcmi_kmeans_mind2_dev: bad argument");
  if (N > 0)
    VCMI_HIP(hipMemcpyAsync(dmind2, h->mind2.p, sizeof(double) * N, hipMemcpyDeviceToDevice, vcmi::as_stream(stream)));
  return VCMI_OK;
}
