// dtw_twokernel.hip -- the DTW paths that keep the observation costs or the tables in memory: observation + recurrence kernels
// (cost / back-pointer tables, D > 48, windows other than bstep 1 or 2 with fstep 0) and the generic kernel (any D, any
// length).  The fused path is dtw_fused.hip; dtw.hip (dtw_run) decides between the two.  Compiled with -ffp-contract=off
// like dtw.hip: the bit-exact contract is stated there.
#include "dtw_internal.hpp"
#include "dtw_device.hpp"

namespace vcmi {

// ------------------------------------------------------------------------------------------------
// Fast path = two kernels.
//
// (1) dtw_obs_kernel<DMAX>: the observation costs O[i,t] = sum_d (seq[d,t] - tmpl[d,i])^2 of every cell, which do
//     not depend on the recurrence, are computed with NO barrier: lane = template frame (its D values in VGPRs),
//     the sequence column is wave-uniform and arrives through scalar loads (`feats` is a read-only, non-aliased
//     kernel argument), i.e. as SGPR operands of the FP64 ALU -- no LDS traffic, no per-lane loads.  (An LDS-staged
//     broadcast variant measured 2x slower than per-lane loads: the LDS pipe, not the FP64 ALU, became the limiter.)
//     Arithmetic order: sequential in d, unfused sub / mul / add (bit-exact contract).  O goes to an HBM workspace
//     in the cost table's (S,T) column-major order, so writes and the later reads are coalesced.
// (2) dtw_rec_kernel<STEPS,CODES>: one workgroup per pair, thread r = template frame r: per column a handful of
//     instructions (candidate costs, strict '<' selection in the reference's scan order), previous column
//     double-buffered in LDS, one barrier per column, O prefetched PF columns ahead in registers.
//     STEPS: 1 = (bstep 1, fstep 0), 2 = (bstep 2, fstep 0) -- candidate window unrolled; 0 = run-time window.
//     CODES: 0 = 2-bit step codes in LDS, 1 = byte codes in LDS, 2 = byte codes in HBM.
// ------------------------------------------------------------------------------------------------
static constexpr int kObsRows = 256;    // template frames per obs workgroup (4 waves)
static constexpr int kObsCols = 128;    // sequence frames per obs workgroup

// Observation kernels.  `base` + P.<off>: feature matrices with exactly DMAX doubles per frame (the caller's buffer
// when D == DMAX, else the zero-padded copies made by dtw_pad_kernel).
//
// Compiler-scheduled variant (DMAX > 40): RPL template frames per lane (a wave owns 64*RPL consecutive frames), so
// that every scalar-loaded sequence value feeds RPL subtractions.
template <int DMAX, int RPL>
__global__ void __launch_bounds__(kObsRows)
dtw_obs_kernel(const double *__restrict__ base, int padded, const DtwPair *__restrict__ pairs, double *__restrict__ obs_ws) {
  const DtwPair P = pairs[blockIdx.x];
  const int S = P.S, T = P.T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rbase = (blockIdx.y * (kObsRows / 64) + wave) * (64 * RPL);
  const int t0 = blockIdx.z * kObsCols;
  if (rbase >= S || t0 >= T) return;                          // wave-uniform (no barriers in this kernel)
  const double *__restrict__ seq = base + (padded ? P.spad_off : P.seq_off);
  const double *__restrict__ tmpl = base + (padded ? P.tpad_off : P.tmpl_off);
  double tm[RPL][DMAX];
  bool active[RPL];
#pragma unroll
  for (int q = 0; q < RPL; ++q) {
    const int r = rbase + 64 * q + lane;
    active[q] = r < S;
    const double *row = tmpl + (int64_t)DMAX * (active[q] ? r : S - 1);
#pragma unroll
    for (int d = 0; d < DMAX; ++d) tm[q][d] = row[d];
  }
  const int t1 = (t0 + kObsCols < T) ? t0 + kObsCols : T;
  double *__restrict__ O = obs_ws + P.obs_off + rbase + lane;   // kernel-argument base: global (not flat) stores
  for (int t = t0; t < t1; ++t) {
    const double *__restrict__ v = seq + (size_t)DMAX * t;     // wave-uniform -> scalar loads
    double o[RPL];                                              // observation(d, v, i), src/dtw.jl:33-35
#pragma unroll
    for (int q = 0; q < RPL; ++q) o[q] = 0.0;
#pragma unroll
    for (int d = 0; d < DMAX; ++d)
#pragma unroll
      for (int q = 0; q < RPL; ++q) {
        const double df = v[d] - tm[q][d];
        const double sq = df * df;
        o[q] = o[q] + sq;
      }
#pragma unroll
    for (int q = 0; q < RPL; ++q)
      if (active[q]) O[(size_t)S * t + 64 * q] = o[q];
  }
}

// Hand-scheduled column loop (tools/gen_dtw_obs_asm.py -> dtw_obs_asm.inc), DMAX <= 40: lane = template frame (its
// DMAX values in v[0:2*DMAX-1]), the sequence column arrives through scalar loads in half-column chunks with two SGPR
// buffers -- wait(0) -> issue the next chunk's loads -> FP64 work of the current chunk -- see the generator for why the
// compiler cannot produce this schedule.  91 VGPRs -> 5 waves per SIMD.
#include "dtw_obs_asm.inc"
template <int DMAX>
__global__ void __launch_bounds__(kObsRows)
dtw_obs_asm_kernel(const double *__restrict__ base, int padded, const DtwPair *__restrict__ pairs,
                   double *__restrict__ obs_ws) {
  const DtwPair P = pairs[blockIdx.x];
  const int S = P.S, T = P.T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rbase = (blockIdx.y * (kObsRows / 64) + wave) * 64;
  const int t0 = blockIdx.z * kObsCols;
  if (rbase >= S || t0 >= T) return;                        // wave-uniform (no barriers in this kernel)
  const int t1 = (t0 + kObsCols < T) ? t0 + kObsCols : T;
  const int r0 = rbase + lane;
  // rows past the template are clamped for the loads and masked for the stores
  const double *row0 = base + (padded ? P.tpad_off : P.tmpl_off) + (int64_t)DMAX * (r0 < S ? r0 : S - 1);
  const double *seq = base + (padded ? P.spad_off : P.seq_off) + (int64_t)DMAX * t0;   // wave-uniform
  double *optr = obs_ws + P.obs_off + (int64_t)S * t0 + r0;
  const uint64_t m0 = __ballot(r0 < S);
  const uint64_t stride = (uint64_t)S * 8;
  uint32_t ncols = (uint32_t)(t1 - t0), off = 0;
  // Warm this XCD's L2 with the workgroup's block of sequence columns (one vector load per 64-byte line, all in flight
  // at once): a scalar load has one chunk of lead time, which covers an L2 hit but not an HBM / Infinity-Cache miss.
  double pf = 0.0;
  const int nlines = (int)ncols * DMAX / 8;
  for (int l = threadIdx.x; l < nlines; l += kObsRows) pf += seq[8 * l];
#define VCMI_OBS_ASM(BODY)                                                                                          \
  asm volatile(BODY                                                                                                 \
               : [seq] "+s"(seq), [n] "+s"(ncols), [optr] "+v"(optr), [off] "+s"(off)                               \
               : [row0] "v"(row0), [stride] "s"(stride), [m0] "s"(m0)                                               \
               : "memory", "vcc", "scc", VCMI_OBS_ASM_CLOBBERS)
  if constexpr (DMAX == 8) VCMI_OBS_ASM(VCMI_DTW_OBS_ASM_D8);
  if constexpr (DMAX == 16) VCMI_OBS_ASM(VCMI_DTW_OBS_ASM_D16);
  if constexpr (DMAX == 24) VCMI_OBS_ASM(VCMI_DTW_OBS_ASM_D24);
  if constexpr (DMAX == 32) VCMI_OBS_ASM(VCMI_DTW_OBS_ASM_D32);
  if constexpr (DMAX == 40) VCMI_OBS_ASM(VCMI_DTW_OBS_ASM_D40);
#undef VCMI_OBS_ASM
  if (pf == 0x1.123456789abcdp+1000) obs_ws[0] = pf;   // keeps the warm-up loads alive; never true for finite features
}

// The dynamic LDS of dtw_rec_kernel, which declares it again in its body without an alignment: the alignment given here is
// what places the array on a 16-byte boundary, 208 bytes behind the static __shared__ of the epilogue (200 without it).  The
// kernel's measured code has every LDS address at that start (profiles/dtw_split/README.md).
extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];

template <int STEPS, int CODES>
__global__ void __launch_bounds__(1024)
dtw_rec_kernel(const double *__restrict__ feats, const DtwPair *__restrict__ pairs, int D, int fstep, int bstep, int Smax,
               int Tmax, const double *__restrict__ obs_ws) {
  constexpr bool LDSCODES = (CODES != 2);
  constexpr int BITS = (CODES == 0) ? 2 : 8;
  constexpr int CPW = 32 / BITS;
  constexpr int PF = 8;                                   // columns of O per register set
  // This kernel is a chain of ~T short dependent steps; observation kernels of the next chunk run beside it on the same
  // CUs (dtw_run) and must not delay its instruction issue.
  __builtin_amdgcn_s_setprio(3);
  const DtwPair P = pairs[blockIdx.x];
  const int S = P.S, T = P.T;
  const int r = threadIdx.x;
  const bool active = r < S;
  extern __shared__ unsigned char smem_raw[];
  double *cbuf = reinterpret_cast<double *>(smem_raw);            // [2][Smax]
  int32_t *path32 = reinterpret_cast<int32_t *>(cbuf + 2 * Smax); // [Tmax]
  int32_t *owner = path32 + Tmax;                                 // [Smax]
  int32_t *holes = owner + Smax;                                  // [Smax]
  uint32_t *codes = reinterpret_cast<uint32_t *>(holes + Smax);   // [ceil(Tmax/CPW)][Smax] when LDSCODES
  if (T == 0) return;
  // kernel-argument base -> global_load with counted vmcnt (a pointer loaded from the descriptor would be a FLAT
  // load, which must be waited for with vmcnt(0) and would serialise the prefetch)
  const double *__restrict__ O = obs_ws + P.obs_off;

  // lazy_init!: costtable[:,1] = 1:S, backpointer[:,1] = 1:S  (src/dtw.jl:49-50)
  double cprev = (double)(r + 1);
  if (active) {
    cbuf[r] = cprev;
    if (P.cost) P.cost[r] = cprev;
    if (P.bp) P.bp[r] = r + 1;
  }
  // O is read PF columns at a time into one of two register sets (ping-pong, unconditional clamped loads issued as
  // a batch) while the other set is consumed, so HBM latency is covered by PF columns of recurrence work.
  const int rl = active ? r : 0;
  auto load_set = [&](double (&dst)[PF], int tbase) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      int tc = tbase + k;
      tc = tc < T ? tc : T - 1;
      dst[k] = O[(size_t)S * tc + rl];
    }
  };
  uint32_t word = 0;
  auto column = [&](int t, double o) {
    const double *cp = cbuf + (t & 1) * Smax;
    double *cn = cbuf + ((t + 1) & 1) * Smax;
    if (active) {
      int arg = r;                                    // minindex = i, src/dtw.jl:106-110
      double best = (cprev + o) + 1.0;
      if (STEPS == 0) {
        for (int j = r - bstep; j <= r + fstep; ++j) {  // src/dtw.jl:113-121
          if (j < 0 || j >= S) continue;
          const double c = (cp[j] + o) + dtw_transition(j, r);
          if (c < best) { best = c; arg = j; }
        }
      } else {
        // window j = r-STEPS .. r, increasing j; j == r repeats the start value and never wins the strict '<'
        if (STEPS == 2) {
          const double c2 = (cp[r >= 2 ? r - 2 : r] + o) + 2.0;
          if (r >= 2 && c2 < best) { best = c2; arg = r - 2; }
        }
        const double c1 = (cp[r >= 1 ? r - 1 : r] + o) + 0.0;
        if (r >= 1 && c1 < best) { best = c1; arg = r - 1; }
      }
      cn[r] = best;
      cprev = best;
      if (P.cost) P.cost[(size_t)S * (t + 1) + r] = best;
      if (P.bp) P.bp[(size_t)S * (t + 1) + r] = arg + 1;
      const uint32_t code = (uint32_t)(r - arg + fstep);
      if (LDSCODES) {
        word |= code << (BITS * (t % CPW));
        if ((t % CPW) == CPW - 1 || t == T - 1) {
          codes[(t / CPW) * Smax + r] = word;
          word = 0;
        }
      } else {
        P.codes[(size_t)S * t + r] = (unsigned char)code;
      }
    }
    // column barrier that waits for the LDS traffic only: __syncthreads() would also drain vmcnt, i.e. stall every
    // column on the O prefetches that are meant to stay in flight
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  double oa[PF], ob[PF];
  load_set(oa, 0);
  __syncthreads();
  for (int t0 = 0; t0 < T; t0 += 2 * PF) {
    load_set(ob, t0 + PF);
#pragma unroll
    for (int k = 0; k < PF; ++k)
      if (t0 + k < T) column(t0 + k, oa[k]);              // wave-uniform guard
    load_set(oa, t0 + 2 * PF);
#pragma unroll
    for (int k = 0; k < PF; ++k)
      if (t0 + PF + k < T) column(t0 + PF + k, ob[k]);
  }
  if (!LDSCODES) {      // the codes in HBM were written by this workgroup: workgroup scope (an agent-scope fence is L2-wide)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  dtw_finish<LDSCODES, BITS>(P, feats + P.seq_off, D, fstep, cbuf + (T & 1) * Smax, path32, owner, holes, codes, Smax);
}

// ------------------------------------------------------------------------------------------------
// Generic kernel: any D, S up to the LDS capacity of two cost columns; rows strided over threads,
// template read from HBM/L2, step codes as bytes in HBM.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
dtw_generic_kernel(const double *__restrict__ feats, const DtwPair *__restrict__ pairs, int D, int fstep, int bstep, int Smax, int Tmax,
                   unsigned char *__restrict__ gscr, size_t gscr_stride) {
  // gscr (templates beyond ~5800 frames: two cost columns, the path and the align() lists no longer fit LDS): the same
  // arrays in a per-pair HBM scratch -- the reference has no length limit (src/dtw.jl:11-59); __syncthreads orders the
  // workgroup's global accesses as it orders its LDS accesses
  const DtwPair P = pairs[blockIdx.x];
  const int S = P.S, T = P.T, tid = threadIdx.x, nthr = blockDim.x;
  extern __shared__ unsigned char smem_lds[];
  unsigned char *smem_raw = gscr ? gscr + (size_t)blockIdx.x * gscr_stride : smem_lds;
  double *cbuf = reinterpret_cast<double *>(smem_raw);
  int32_t *path32 = reinterpret_cast<int32_t *>(cbuf + 2 * Smax);
  int32_t *owner = path32 + Tmax;
  int32_t *holes = owner + Smax;
  if (T == 0) return;
  for (int r = tid; r < S; r += nthr) {
    cbuf[r] = (double)(r + 1);
    if (P.cost) P.cost[r] = (double)(r + 1);
    if (P.bp) P.bp[r] = r + 1;
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const double *cp = cbuf + (t & 1) * Smax;
    double *cn = cbuf + ((t + 1) & 1) * Smax;
    const double *__restrict__ v = feats + P.seq_off + (size_t)D * t;
    for (int r = tid; r < S; r += nthr) {
      const double *__restrict__ tc = feats + P.tmpl_off + (size_t)D * r;
      double o = 0.0;
      for (int d = 0; d < D; ++d) {
        const double df = v[d] - tc[d];
        const double sq = df * df;
        o = o + sq;
      }
      int arg = r;
      double best = (cp[r] + o) + 1.0;
      for (int j = r - bstep; j <= r + fstep; ++j) {
        if (j < 0 || j >= S) continue;
        const double c = (cp[j] + o) + dtw_transition(j, r);
        if (c < best) { best = c; arg = j; }
      }
      cn[r] = best;
      if (P.cost) P.cost[(size_t)S * (t + 1) + r] = best;
      if (P.bp) P.bp[(size_t)S * (t + 1) + r] = arg + 1;
      P.codes[(size_t)S * t + r] = (unsigned char)(r - arg + fstep);
    }
    __syncthreads();
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  dtw_finish<false, 8>(P, feats + P.seq_off, D, fstep, cbuf + (T & 1) * Smax, path32, owner, holes, nullptr, Smax);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int launch_rec(const double *feats, const DtwPair *dpairs, int n, int D, int fstep, int bstep, int Smax, int Tmax,
                      int steps, int codes, size_t shmem, int threads, const double *obs_ws, hipStream_t st) {
#define VCMI_DTW_LAUNCH(ST, CO)                                                                                \
  do {                                                                                                         \
    auto kern = dtw_rec_kernel<ST, CO>;                                                                        \
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                 (int)shmem));                                                                 \
    hipLaunchKernelGGL(kern, dim3(n), dim3(threads), shmem, st, feats, dpairs, D, fstep, bstep, Smax, Tmax, obs_ws); \
  } while (0)
  if (steps == 1 && codes == 0) VCMI_DTW_LAUNCH(1, 0);
  else if (steps == 1) VCMI_DTW_LAUNCH(1, 2);
  else if (steps == 2 && codes == 0) VCMI_DTW_LAUNCH(2, 0);
  else if (steps == 2) VCMI_DTW_LAUNCH(2, 2);
  else if (codes == 0) VCMI_DTW_LAUNCH(0, 0);
  else if (codes == 1) VCMI_DTW_LAUNCH(0, 1);
  else VCMI_DTW_LAUNCH(0, 2);
#undef VCMI_DTW_LAUNCH
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// Side stream on which the observation kernels run: the recurrence of chunk c (latency-bound: one barrier per column,
// few FP64 instructions) overlaps the observation costs of chunk c+1 (FP64-ALU-bound) on the same CUs.
struct DtwOverlap {
  static constexpr int kMaxChunks = 8;
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, done[kMaxChunks] = {};
  int device = -1;
  int init() {
    int dev = 0;
    VCMI_HIP(hipGetDevice(&dev));
    if (side && dev == device) return VCMI_OK;
    release();
    VCMI_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    VCMI_HIP(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
    for (auto &e : done) VCMI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    device = dev;
    return VCMI_OK;
  }
  void release() {
    if (side) (void)hipStreamDestroy(side);
    if (fork) (void)hipEventDestroy(fork);
    for (auto &e : done)
      if (e) (void)hipEventDestroy(e);
    side = nullptr;
    fork = nullptr;
    for (auto &e : done) e = nullptr;
  }
  ~DtwOverlap() { release(); }
};
static DtwOverlap &dtw_overlap() {
  static thread_local DtwOverlap o;
  return o;
}

static int launch_obs(const double *feats, const double *spad, const DtwPair *dpairs, int n, int D, int Smax, int Tmax,
                      double *obs_ws, hipStream_t st) {
  const int dmax = dtw_dmax(D);
  const int padded = (D != dmax);
  const double *sbase = padded ? spad : feats;
  if (padded) dtw_launch_pad(feats, dpairs, n, D, dmax, const_cast<double *>(spad), st);
  const unsigned colblocks = (Tmax + kObsCols - 1) / kObsCols;
  if (dmax <= 40) {   // hand-scheduled column loop, one template frame per lane (5 waves per SIMD)
    const dim3 grid(n, (Smax + kObsRows - 1) / kObsRows, colblocks);
#define VCMI_OBS_CASE(DM) \
  case DM: hipLaunchKernelGGL((dtw_obs_asm_kernel<DM>), grid, dim3(kObsRows), 0, st, sbase, padded, dpairs, obs_ws); break;
    switch (dmax) { VCMI_OBS_CASE(8) VCMI_OBS_CASE(16) VCMI_OBS_CASE(24) VCMI_OBS_CASE(32) VCMI_OBS_CASE(40) }
#undef VCMI_OBS_CASE
  } else {            // compiler-scheduled loop (two frames per lane at DMAX = 48 spills SGPRs: one frame per lane)
    const dim3 grid(n, (Smax + kObsRows - 1) / kObsRows, colblocks);
    switch (dmax) {
      case 48: hipLaunchKernelGGL((dtw_obs_kernel<48, 1>), grid, dim3(kObsRows), 0, st, sbase, padded, dpairs, obs_ws); break;
      case 64: hipLaunchKernelGGL((dtw_obs_kernel<64, 1>), grid, dim3(kObsRows), 0, st, sbase, padded, dpairs, obs_ws); break;
      default: hipLaunchKernelGGL((dtw_obs_kernel<96, 1>), grid, dim3(kObsRows), 0, st, sbase, padded, dpairs, obs_ws); break;
    }
  }
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

// Everything dtw_run does not give to the fused path: slices of at most ~4 GiB of observation costs, each in chunks whose
// observation kernels run on the side stream, or the generic kernel on LDS or on an HBM scratch.  Launches one workgroup per
// pair; the step codes go to the grow-only sc.codes when they do not fit in LDS.
int dtw_run_twokernel(const double *feats, std::vector<DtwPair> &pairs, int D, int fstep, int bstep, DtwScratch &sc,
                      hipStream_t st, int Smax, int Tmax) {
  DevBuf<unsigned char> &codes_ws = sc.codes;
  DevBuf<double> &obs_ws = sc.obs, &spad_ws = sc.spad;
  DevBuf<DtwPair> &dpairs = sc.dpairs;
  const int n = (int)pairs.size();
  // largest pairs first: shortens the tail when n is not a multiple of the resident workgroup count
  std::stable_sort(pairs.begin(), pairs.end(), [](const DtwPair &a, const DtwPair &b) {
    return (int64_t)a.S * a.T > (int64_t)b.S * b.T;
  });
  const int bits = (fstep + bstep + 1 <= 4) ? 2 : 8;
  const size_t base = (size_t)2 * Smax * 8 + (size_t)Tmax * 4 + (size_t)2 * Smax * 4;
  const size_t base_generic = base;
  // two cost columns + path + lists beyond LDS (a template of > ~5800 frames, or a SEQUENCE of > ~34k frames whatever the
  // template: the path alone is 4 T bytes): the generic kernel on an HBM scratch -- the two-kernel fast path keeps them in LDS
  const bool longseq = base > kLdsLimit;
  const bool fast = (Smax <= 1024 && D <= 96 && !longseq);
  const size_t codes_lds = (size_t)((Tmax + (32 / bits) - 1) / (32 / bits)) * Smax * 4;
  const bool ldscodes = fast && (base + codes_lds <= kLdsLimit);
  if (!ldscodes) {
    size_t total = 0;
    for (auto &p : pairs) total += (size_t)p.S * p.T;
    VCMI_TRY(codes_ws.reserve(total));
    size_t off = 0;
    for (auto &p : pairs) {
      p.codes = codes_ws.p + off;
      off += (size_t)p.S * p.T;
    }
  }
  VCMI_TRY(dpairs.reserve(n));
  if (fast) {
    // observation-cost workspace: S*T doubles per pair; large batches run in slices of at most ~4 GiB
    const int threads = (Smax + 63) / 64 * 64;
    const size_t shmem = base + (ldscodes ? codes_lds : 0);
    const int steps = (fstep == 0 && bstep == 1) ? 1 : (fstep == 0 && bstep == 2) ? 2 : 0;
    const int codes = !ldscodes ? 2 : (bits == 2 ? 0 : 1);
    const size_t kMaxCells = (size_t)1 << 29;
    int lo = 0;
    while (lo < n) {
      size_t cells = 0;
      int hi = lo;
      while (hi < n && (hi == lo || cells + (size_t)pairs[hi].S * pairs[hi].T <= kMaxCells)) {
        cells += (size_t)pairs[hi].S * pairs[hi].T;
        ++hi;
      }
      VCMI_TRY(obs_ws.reserve(cells));
      const int dmax = dtw_dmax(D);
      if (D != dmax) {
        size_t padn = 0;
        for (int k = lo; k < hi; ++k) padn += (size_t)(pairs[k].T + pairs[k].S) * dmax;
        VCMI_TRY(spad_ws.reserve(padn));
      }
      size_t off = 0, poff = 0;
      int smax = 0, tmax = 0;
      for (int k = lo; k < hi; ++k) {
        pairs[k].obs_off = (int64_t)off;
        off += (size_t)pairs[k].S * pairs[k].T;
        pairs[k].spad_off = (int64_t)poff;
        poff += (size_t)pairs[k].T * dmax;
        pairs[k].tpad_off = (int64_t)poff;
        poff += (size_t)pairs[k].S * dmax;
        smax = std::max(smax, pairs[k].S);
        tmax = std::max(tmax, pairs[k].T);
      }
      VCMI_TRY(sc.upload(dpairs.p + lo, pairs.data() + lo, (size_t)(hi - lo), st));
      if (tmax > 0) {
        // chunks of the slice: observation costs on the side stream, recurrences on the caller's stream behind them
        const int m = hi - lo;
        // (a recurrence launch occupies one CU per pair for ~T barriers whatever its size: chunks of about one pair
        // per CU keep every recurrence round full)
        const int nchunks = (m < 192) ? 1 : std::min(DtwOverlap::kMaxChunks, (m + 255) / 256);
        if (nchunks == 1) {
          VCMI_TRY(launch_obs(feats, spad_ws.p, dpairs.p + lo, m, D, smax, tmax, obs_ws.p, st));
          VCMI_TRY(launch_rec(feats, dpairs.p + lo, m, D, fstep, bstep, Smax, Tmax, steps, codes, shmem, threads, obs_ws.p, st));
        } else {
          DtwOverlap &ov = dtw_overlap();
          VCMI_TRY(ov.init());
          VCMI_HIP(hipEventRecord(ov.fork, st));                 // the side stream starts behind the caller's earlier work
          VCMI_HIP(hipStreamWaitEvent(ov.side, ov.fork, 0));     // (which includes the previous call's recurrences)
          for (int c = 0; c < nchunks; ++c) {
            const int c0 = lo + (int)((int64_t)m * c / nchunks), c1 = lo + (int)((int64_t)m * (c + 1) / nchunks);
            VCMI_TRY(launch_obs(feats, spad_ws.p, dpairs.p + c0, c1 - c0, D, smax, tmax, obs_ws.p, ov.side));
            VCMI_HIP(hipEventRecord(ov.done[c], ov.side));
            VCMI_HIP(hipStreamWaitEvent(st, ov.done[c], 0));
            VCMI_TRY(launch_rec(feats, dpairs.p + c0, c1 - c0, D, fstep, bstep, Smax, Tmax, steps, codes, shmem, threads, obs_ws.p, st));
          }
        }
      }
      if (hi < n) VCMI_HIP(hipStreamSynchronize(st));   // the next slice reuses the workspace
      lo = hi;
    }
  } else {
    VCMI_TRY(sc.upload(dpairs.p, pairs.data(), (size_t)n, st));
    if (longseq) {
      const size_t stride = (base_generic + 255) / 256 * 256;
      VCMI_TRY(sc.longscr.reserve((size_t)n * stride));
      hipLaunchKernelGGL(dtw_generic_kernel, dim3(n), dim3(1024), 0, st, feats, dpairs.p, D, fstep, bstep, Smax, Tmax, sc.longscr.p, stride);
    } else {
      VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(dtw_generic_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)base_generic));
      hipLaunchKernelGGL(dtw_generic_kernel, dim3(n), dim3(1024), base_generic, st, feats, dpairs.p, D, fstep, bstep, Smax, Tmax,
                         (unsigned char *)nullptr, (size_t)0);
    }
    VCMI_HIP(hipGetLastError());
  }
  VCMI_HIP(hipEventRecord(sc.last_use, st));
  return VCMI_OK;
}

}  // namespace vcmi
