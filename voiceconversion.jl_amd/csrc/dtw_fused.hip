// dtw_fused.hip -- the fused DTW path: forward kernels (observation costs + recurrence in one), backward and align kernels,
// and their host routine.  Which job waits on which flag is planned by dtw_plan.cpp; dtw.hip (dtw_run) decides whether a call
// comes here.  Compiled with -ffp-contract=off like dtw.hip: the bit-exact contract is stated there.
#include "dtw_internal.hpp"
#include "dtw_device.hpp"

#include <algorithm>

namespace vcmi {

// ------------------------------------------------------------------------------------------------
// Fused path (fstep = 0, bstep in {1,2}, D <= 40, path-only): ONE forward kernel computes observation costs and the
// recurrence together -- O never exists in memory -- and streams the 2-bit step codes to HBM (62.5 KB per 500x500 pair,
// against 2 MB for O); a short second kernel per pair loads the pair's codes into LDS and runs backward + align.
//
// dtw_fused_kernel<DMAX,STEPS>: workgroup = one row strip (<= 512 rows) of a pair = up to 4 waves; a wave owns 128
// consecutive rows, lane l the rows 2l and 2l+1 (their features stay in 160 VGPRs); the sequence column is the wave-
// uniform SGPR operand.  The column loop is hand-scheduled (tools/gen_dtw_fused_asm.py -> dtw_fused_asm.inc, where the
// schedule, the register map and the arithmetic order are documented).  No workgroup barrier inside the loop: the only
// coupling between waves is "lane 0 needs the previous wave's top two rows of the previous column", handed over through
// a sequence-tagged ring in LDS.  LDS use is ~9 KB + 16 B per column, so occupancy is set by the registers (2 waves per
// SIMD = two workgroups per CU).
// ------------------------------------------------------------------------------------------------
#include "dtw_fused_asm.inc"
static constexpr int kFusedThreads = 256;     // (kFusedRows, the rows per strip: dtw_plan.hpp)

// wave-uniform value held in VGPRs -> SGPRs (inline-asm "s" operands)
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint32_t lds_addr(const void *p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char *)p;
}

#ifdef VCMI_DTW_PROF
__device__ unsigned long long dtw_prof[8];      // cycles summed over jobs: [0] prologue, [1] column loop (incl. the template loads), [2] epilogue, [3] jobs, [4] flag waits
#define DTW_PROF_MARK(var) const long long var = (long long)__builtin_readcyclecounter()
#else
#define DTW_PROF_MARK(var)
#endif
// Synchronisation between jobs of the fused kernel (strip below -> strip above, column segment -> next segment).
// The L2 caches of the eight XCDs are not coherent with each other, so an acquire / release at agent scope is an L2-WIDE
// invalidate / write-back (buffer_inv sc1 / buffer_wbl2 sc1) -- which every other workgroup of the XCD pays for: with one
// such pair per job a 100-column job took 325k cycles instead of 240k (cycle counter, VCMI_DTW_PROF).  Instead the few
// values that cross jobs -- boundary pairs, last cost columns, flags -- are themselves accessed at agent scope (sc1: stores
// write through to the device-wide coherence point, loads do not use a possibly stale cached copy), relaxed, and ordered by
// hand: the producer waits until its stores are acknowledged (vmcnt(0)), then stores the flag; the consumer sees the flag,
// then loads.  Everything else a job writes (step codes) is read by a later kernel.
__device__ __forceinline__ void dtw_store_shared(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double dtw_load_shared(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void dtw_wait_flag(const int *flag, int epoch) {
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) __builtin_amdgcn_s_sleep(32);
}
// all of this wave's stores have been acknowledged
__device__ __forceinline__ void dtw_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <int DMAX, int STEPS>
__device__ __forceinline__ void dtw_fused_job(const int sfirst, const double *__restrict__ base, int padded,
                                              const DtwPair *__restrict__ pairs, const DtwStrip *__restrict__ strips,
                                              uint32_t *__restrict__ fcodes_ws, double *__restrict__ bnd_ws,
                                              double *__restrict__ clast_ws, int *__restrict__ flags, int epoch) {
  DTW_PROF_MARK(pt0);
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  unsigned char *outbox = fsm;                                                        // [4][VCMI_FUSED_OUTBOX]
  double *clast = reinterpret_cast<double *>(fsm + 4 * VCMI_FUSED_OUTBOX);            // [kFusedRows]
  double *pinit = clast + kFusedRows;                                                 // [kFusedRows] (DMAX > 40: initial neighbour costs)
  double *bnd = pinit + kFusedRows;                                                   // [1 + T][2]
  // A job is one strip segment (first descriptor `sfirst`), or a PACKED group: each of the four waves runs its own
  // one-wave strip (the short bottom strips of long templates, <= 128 rows), four unrelated strips per workgroup, so that
  // no wave slot idles beside them.
  const int tid = threadIdx.x, lane = tid & 63;
  const bool packed = strips[sfirst].packed != 0;
  const int slotw = tid >> 6;                                  // wave slot in the workgroup (outbox, clast area)
  const DtwStrip st = packed ? strips[sfirst + slotw] : strips[sfirst];
  const DtwPair P = pairs[st.pair];
  const int S = P.S, T = st.ncol, col0 = st.col0;              // T: the columns of THIS job
  if (!packed && T == 0) return;
  const int wave = packed ? 0 : slotw;                         // wave index within the strip
  const int nw = (st.nrows + 127) >> 7;
  const int lr0 = 128 * wave + 2 * lane;            // first row of the lane, local to the strip
  const int gr0 = st.row0 + lr0;                    // ... and in the pair
  // lazy_init!: costtable[:,1] = 1:S (src/dtw.jl:49); the neighbours of column 1 are rows gr0-2, gr0-1
  double c0 = (double)(gr0 + 1), c1 = (double)(gr0 + 2);
  double p0 = gr0 >= 2 ? (double)(gr0 - 1) : INFINITY, p1 = gr0 >= 1 ? (double)gr0 : INFINITY;
  if (__syncthreads_or(st.flag_prev >= 0)) {   // (a packed group: any of its four strips)
    // a later column segment: the previous one (an earlier job: running or finished) left the costs of its last column,
    // for every row of the strip, in clast_ws; rows below the strip belong to the strip below and reach lane 0 of wave 0
    // through the boundary array, like every column's
    if (lane == 0 && (packed || tid == 0) && st.flag_prev >= 0)
      dtw_wait_flag(&flags[st.flag_prev], epoch);
    __syncthreads();
  }
  DTW_PROF_MARK(ptw);
  if (st.flag_prev >= 0) {
    const double *cl = clast_ws + P.clast_off;
    const int last = S - 1;
    c0 = dtw_load_shared(cl + (gr0 < S ? gr0 : last));
    c1 = dtw_load_shared(cl + (gr0 + 1 < S ? gr0 + 1 : last));
    p0 = (gr0 - 2 >= st.row0) ? dtw_load_shared(cl + (gr0 - 2 < S ? gr0 - 2 : last)) : INFINITY;
    p1 = (gr0 - 1 >= st.row0) ? dtw_load_shared(cl + (gr0 - 1 < S ? gr0 - 1 : last)) : INFINITY;
  }
  if (tid < 4) *reinterpret_cast<uint32_t *>(outbox + tid * VCMI_FUSED_OUTBOX + VCMI_FUSED_RING * 16) = 0u;   // tags
  if (lane == 63) {   // what the next wave's lane 0 reads for column 0: the ring's last slot holds the initial costs
    double *slot = reinterpret_cast<double *>(outbox + slotw * VCMI_FUSED_OUTBOX + (VCMI_FUSED_RING - 1) * 16);
    slot[0] = c0;
    slot[1] = c1;
  }
  if (!packed && st.flag_in >= 0) {
    // the strip below must be complete (it precedes this workgroup in the grid, so it is resident or finished)
    if (tid == 0)
      dtw_wait_flag(&flags[st.flag_in], epoch);
    __syncthreads();
    // entry 0: initial costs of the two rows below the strip; entry 1+t: their costs after column t
    // (of this job's columns: LDS entry e <-> the pair's entry col0 + e)
    const double *src = bnd_ws + st.bnd_in + 2 * (int64_t)col0;
    if (tid == 0) {
      bnd[0] = col0 == 0 ? (double)(st.row0 - 1) : dtw_load_shared(src - 2);
      bnd[1] = col0 == 0 ? (double)st.row0 : dtw_load_shared(src - 1);
    }
    for (int i = tid; i < 2 * T; i += (int)blockDim.x) bnd[2 + i] = dtw_load_shared(src + i);
  }
  __syncthreads();
  DTW_PROF_MARK(pt1);
  if (wave < nw && T > 0) {
    // (the 40 loads of a lane's two rows touch 64 cache lines each; measured, they cost nothing: a packed, fully coalesced
    // copy of the templates left the job time unchanged and its packing kernel took 85 us)
    const double *tmpl = base + (padded ? P.tpad_off : P.tmpl_off);
    const double *rowA = tmpl + (int64_t)DMAX * (gr0 < S ? gr0 : S - 1);
    const double *rowB = tmpl + (int64_t)DMAX * (gr0 + 1 < S ? gr0 + 1 : S - 1);
    const double *seq = base + (padded ? P.spad_off : P.seq_off) + (int64_t)DMAX * col0;
    const int Se = (S + 1) & ~1;
    uint32_t *codes = fcodes_ws + P.fcodes_off + gr0 + (int64_t)(col0 >> 4) * Se;
    const uint64_t cstride = (uint64_t)Se * 4;
    int cnt = (st.nrows - 128 * wave + 1) >> 1;
    cnt = cnt > 64 ? 64 : cnt;
    uint32_t out = lds_addr(outbox + slotw * VCMI_FUSED_OUTBOX), bndl = lds_addr(bnd);
    uint32_t mode = (wave > 0 ? 1u : 0u) | ((wave == 0 && !packed && st.flag_in >= 0) ? 2u : 0u) | (wave + 1 < nw ? 4u : 0u);
    int explane = -1;
    double *gout = bnd_ws;
    if (st.bnd_out >= 0 && wave == nw - 1) {          // non-final strips have an even number of rows
      explane = (st.nrows >> 1) - 1 - 64 * wave;
      gout = bnd_ws + st.bnd_out + 2 * (int64_t)col0;
    }
    uint32_t clast_a = lds_addr(clast + 128 * slotw + 2 * lane);
    if constexpr (DMAX > 40) {     // the wide kernels read their initial costs from LDS (operand VGPRs are scarce there)
      clast[128 * slotw + 2 * lane] = c0;
      clast[128 * slotw + 2 * lane + 1] = c1;
      pinit[128 * slotw + 2 * lane] = p0;
      pinit[128 * slotw + 2 * lane + 1] = p1;
    }
    uint32_t ncols = (uint32_t)T, off = 0, tcol = 0;
    // every operand the loop reads is wave-uniform or per-lane as declared; force the uniform ones into SGPRs
    cnt = __builtin_amdgcn_readfirstlane(cnt);
    out = __builtin_amdgcn_readfirstlane(out);
    bndl = __builtin_amdgcn_readfirstlane(bndl);
    mode = __builtin_amdgcn_readfirstlane(mode);
    explane = __builtin_amdgcn_readfirstlane(explane);
    ncols = __builtin_amdgcn_readfirstlane(ncols);
    seq = reinterpret_cast<const double *>(uniform64(reinterpret_cast<uint64_t>(seq)));
    const uint64_t cstride_u = uniform64(cstride);
#define VCMI_FUSED_ASM(BODY) VCMI_FUSED_ASM_C(BODY, VCMI_FUSED_ASM_CLOBBERS)
#define VCMI_FUSED_ASM_C(BODY, CLOBBERS)                                                                              \
  asm volatile(BODY                                                                                                   \
               : [seq] "+s"(seq), [off] "+s"(off), [n] "+s"(ncols), [t] "+s"(tcol), [codes] "+v"(codes), [gout] "+v"(gout) \
               : [cstride] "s"(cstride_u), [cnt] "s"(cnt), [out] "s"(out), [bnd] "s"(bndl), [mode] "s"(mode),          \
                 [explane] "s"(explane), [rowA] "v"(rowA), [rowB] "v"(rowB), [c0] "v"(c0), [c1] "v"(c1), [p0] "v"(p0), \
                 [p1] "v"(p1), [clast] "v"(clast_a)                                                                   \
               : "memory", "vcc", "scc", CLOBBERS)
    // the wide kernels (40 < D <= 48) read the initial costs from LDS: (C0, C1) at %[clast], (P0, P1) kFusedRows doubles behind
#define VCMI_FUSED3_ASM(BODY, CLOBBERS)                                                                               \
  asm volatile(BODY                                                                                                   \
               : [seq] "+s"(seq), [off] "+s"(off), [n] "+s"(ncols), [t] "+s"(tcol), [codes] "+v"(codes), [gout] "+v"(gout) \
               : [cstride] "s"(cstride_u), [cnt] "s"(cnt), [out] "s"(out), [bnd] "s"(bndl), [mode] "s"(mode),          \
                 [explane] "s"(explane), [rowA] "v"(rowA), [rowB] "v"(rowB), [clast] "v"(clast_a)                      \
               : "memory", "vcc", "scc", CLOBBERS)
    if constexpr (STEPS == 1) {
      if constexpr (DMAX == 8) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D8_S1);
      if constexpr (DMAX == 16) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D16_S1);
      if constexpr (DMAX == 24) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D24_S1);
      if constexpr (DMAX == 32) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D32_S1);
      if constexpr (DMAX == 40) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D40_S1);
      if constexpr (DMAX == 41) VCMI_FUSED3_ASM(VCMI_DTW_FUSED_ASM_D41_S1, VCMI_FUSED_ASM_CLOBBERS_D41);
      if constexpr (DMAX == 48) VCMI_FUSED3_ASM(VCMI_DTW_FUSED_ASM_D48_S1, VCMI_FUSED_ASM_CLOBBERS_D48);
    } else {
      if constexpr (DMAX == 41) VCMI_FUSED3_ASM(VCMI_DTW_FUSED_ASM_D41_S2, VCMI_FUSED_ASM_CLOBBERS_D41);
      if constexpr (DMAX == 48) VCMI_FUSED3_ASM(VCMI_DTW_FUSED_ASM_D48_S2, VCMI_FUSED_ASM_CLOBBERS_D48);
      if constexpr (DMAX == 8) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D8_S2);
      if constexpr (DMAX == 16) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D16_S2);
      if constexpr (DMAX == 24) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D24_S2);
      if constexpr (DMAX == 32) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D32_S2);
#if !defined(VCMI_FUSED_VARIANT)
      if constexpr (DMAX == 40) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D40_S2);
#elif VCMI_FUSED_VARIANT == 1   // timing experiments only (wrong results): see tools/gen_dtw_fused_asm.py
      if constexpr (DMAX == 40) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D40_S2_V1);
#elif VCMI_FUSED_VARIANT == 2
      if constexpr (DMAX == 40) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D40_S2_V2);
#else
      if constexpr (DMAX == 40) VCMI_FUSED_ASM(VCMI_DTW_FUSED_ASM_D40_S2_V3);
#endif
    }
#undef VCMI_FUSED_ASM
#undef VCMI_FUSED_ASM_C
#undef VCMI_FUSED3_ASM
  }
  __syncthreads();
  DTW_PROF_MARK(pt2);
#ifdef VCMI_DTW_PROF
  auto prof_end = [&]() {
    const long long pt3 = (long long)__builtin_readcyclecounter();
    if (tid == 0) {
      atomicAdd(&dtw_prof[0], (unsigned long long)(pt1 - pt0));
      atomicAdd(&dtw_prof[1], (unsigned long long)(pt2 - pt1));
      atomicAdd(&dtw_prof[2], (unsigned long long)(pt3 - pt2));
      atomicAdd(&dtw_prof[3], 1ull);
      atomicAdd(&dtw_prof[4], (unsigned long long)(ptw - pt0));
    }
  };
#endif
  if (packed) {      // every wave finishes its own strip
    if (T > 0) {
      for (int i = lane; i < st.nrows; i += 64) dtw_store_shared(&clast_ws[P.clast_off + st.row0 + i], clast[128 * slotw + i]);
      if (st.flag_out >= 0) {
        dtw_stores_done();      // (also the boundary pairs the column loop exported)
        if (lane == 0) __hip_atomic_store(&flags[st.flag_out], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
#ifdef VCMI_DTW_PROF
    prof_end();
#endif
    return;
  }
  for (int i = tid; i < st.nrows; i += (int)blockDim.x) dtw_store_shared(&clast_ws[P.clast_off + st.row0 + i], clast[i]);
  if (st.flag_out >= 0) {
    dtw_stores_done();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(&flags[st.flag_out], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#ifdef VCMI_DTW_PROF
  prof_end();
#endif
}

// One job per workgroup, in grid order.
template <int DMAX, int STEPS>
__global__ void __launch_bounds__(kFusedThreads)
dtw_fused_kernel(const double *__restrict__ base, int padded, const DtwPair *__restrict__ pairs,
                 const DtwStrip *__restrict__ strips, uint32_t *__restrict__ fcodes_ws, double *__restrict__ bnd_ws,
                 double *__restrict__ clast_ws, int *__restrict__ flags, int epoch, const int *__restrict__ job_first) {
  dtw_fused_job<DMAX, STEPS>(job_first[blockIdx.x], base, padded, pairs, strips, fcodes_ws, bnd_ws, clast_ws, flags, epoch);
}

// Persistent form: as many workgroups as the device holds at once, each drawing the next job from a ticket counter until
// the list is exhausted.  A workgroup that waits on a flag waits for a job with a LOWER ticket (the list is in dependency
// order), i.e. for a job some running workgroup already holds: no deadlock, whatever the residency.  With the columns cut
// into segments the jobs are short; drawing them inside the kernel removes the gap the hardware dispatcher leaves
// between a finished workgroup and its successor.
template <int DMAX, int STEPS>
__global__ void __launch_bounds__(kFusedThreads, 2)      // two workgroups per CU: 256 registers
dtw_fused_persistent_kernel(const double *__restrict__ base, int padded, const DtwPair *__restrict__ pairs,
                            const DtwStrip *__restrict__ strips, uint32_t *__restrict__ fcodes_ws, double *__restrict__ bnd_ws,
                            double *__restrict__ clast_ws, int *__restrict__ flags, int epoch, const int *__restrict__ job_first,
                            int njobs, int *__restrict__ ticket) {
  __shared__ int job_s;
  for (;;) {
    if (threadIdx.x == 0) job_s = atomicAdd(ticket, 1);
    __syncthreads();
    const int job = __builtin_amdgcn_readfirstlane(job_s);     // uniform: the job's descriptors stay in SGPRs
    __syncthreads();                // (job_s is rewritten by the next draw)
    if (job >= njobs) break;
    dtw_fused_job<DMAX, STEPS>(job_first[job], base, padded, pairs, strips, fcodes_ws, bnd_ws, clast_ws, flags, epoch);
    __syncthreads();                // the next job reuses the outboxes, the boundary array and the last-column area
  }
}

// Backward pass of the fused path: ONE WAVE per pair, no LDS.  (Round 2's epilogue copied the pair's 64 KB of packed step
// codes into LDS and let one thread chase T dependent LDS reads: 110 us for 1000 pairs, two workgroups per CU.)  The path
// moves down by at most two rows per column (bstep <= 2, fstep = 0), so over the 16 columns of one code-word row it stays
// within 33 rows: a wave keeps a WINDOW of 192 rows of that word row in three registers per lane (coalesced loads), the
// walk itself is scalar -- v_readlane with the uniform row, shift, mask, subtract -- and the windows of the next three word
// rows are in flight meanwhile (a window anchored at the current row r covers [r - 191, r]; the word row three blocks
// ahead is entered at r - 64 or above and left at r - 96 or above).  Path values are collected one per lane, parked in LDS
// per 64 columns (no global store inside the walk: loads and stores share vmcnt and complete out of order with respect
// to each other, so with a store pending the compiler waits for vmcnt(0) before every block and the look-ahead is lost)
// and leave at the end as coalesced stores: 0-based to path32_ws (for the align kernel), 1-based Int64 to the caller's path.
__device__ __forceinline__ void dtw_window_load(const uint32_t *__restrict__ gc, int Se, int tb, int anchor, int lane, uint32_t (&w)[3]) {
  // (unconditional -- beyond the first word row it re-reads row 0: the compiler can then count the loads in flight, with
  // a conditional load it waits for vmcnt(0) before every block and the look-ahead is lost)
  const uint32_t *rowp = gc + (size_t)(tb < 0 ? 0 : tb) * Se;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int r = anchor - 191 + 64 * k + lane;
    r = r < 0 ? 0 : (r >= Se ? Se - 1 : r);            // (rows the walk cannot reach)
    w[k] = rowp[r];
  }
}

__global__ void __launch_bounds__(64)
dtw_fused_backward_kernel(const DtwPair *__restrict__ pairs, const uint32_t *__restrict__ fcodes_ws,
                          const double *__restrict__ clast_ws, int32_t *__restrict__ path32_ws) {
  extern __shared__ int32_t path_lds[];                 // [Tmax]
  const int lane = threadIdx.x;
  const DtwPair P = pairs[blockIdx.x];
  const int S = P.S, T = P.T;
  if (T == 0) return;
  // indmin of the last column, first minimum wins (src/dtw.jl:137)
  int row;
  {
    const double *cl = clast_ws + P.clast_off;
    double bv = INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < S; i += 64) {
      const double c = cl[i];
      if (c < bv) { bv = c; bi = i; }
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
      const double ov = __shfl_xor(bv, sh);
      const int oi = __shfl_xor(bi, sh);
      if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    row = __builtin_amdgcn_readfirstlane(bi);
  }
  const int Se = (S + 1) & ~1;
  const uint32_t *gc = fcodes_ws + P.fcodes_off;
  int32_t *p32 = path32_ws + P.path32_off;
  int64_t *p64 = P.path;
  int acc = 0;                                          // lane l: path value of column 64 q + l of the current group q
  auto flush = [&](int q) {
    const int col = 64 * q + lane;
    if (col < T) path_lds[col] = acc;
  };
  // path[c] = row, then the code of column c (for c >= 1) leads to path[c - 1] (src/dtw.jl:140-142)
  auto walk = [&](int tb, const uint32_t (&w)[3], int anchor) {
    const int thi = (16 * tb + 15 < T - 1) ? 16 * tb + 15 : T - 1, tlo = (16 * tb > 1) ? 16 * tb : 1;
    for (int t = thi; t >= tlo; --t) {
      const int idx = row - (anchor - 191);
      const int l = idx & 63;
      const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)w[0], l), w1 = (uint32_t)__builtin_amdgcn_readlane((int)w[1], l),
                     w2 = (uint32_t)__builtin_amdgcn_readlane((int)w[2], l);
      const uint32_t word = (idx < 64) ? w0 : ((idx < 128) ? w1 : w2);
      row -= (int)((word >> (2 * (t & 15))) & 3u);
      const int c = t - 1;
      if ((c & 63) == 63) flush((c + 1) >> 6);          // column c opens a new group: the finished one leaves
      acc = (lane == (c & 63)) ? row : acc;
    }
  };
  acc = (lane == ((T - 1) & 63)) ? row : acc;
  uint32_t wa[3] = {0, 0, 0}, wb[3] = {0, 0, 0}, wc[3] = {0, 0, 0};
  int aa = row, ab = row, ac = row;
  int tb = (T - 1) >> 4;
  dtw_window_load(gc, Se, tb, row, lane, wa);
  dtw_window_load(gc, Se, tb - 1, row, lane, wb);
  dtw_window_load(gc, Se, tb - 2, row, lane, wc);
  for (; tb >= 0; tb -= 3) {
    walk(tb, wa, aa);
    aa = row;
    dtw_window_load(gc, Se, tb - 3, row, lane, wa);
    if (tb - 1 < 0) break;
    walk(tb - 1, wb, ab);
    ab = row;
    dtw_window_load(gc, Se, tb - 4, row, lane, wb);
    if (tb - 2 < 0) break;
    walk(tb - 2, wc, ac);
    ac = row;
    dtw_window_load(gc, Se, tb - 5, row, lane, wc);
  }
  flush(0);
  __syncthreads();
  for (int col = lane; col < T; col += 64) {
    const int v = path_lds[col];
    p32[col] = v;
    if (p64) p64[col] = (int64_t)v + 1;
  }
}

// align() of the fused path: one workgroup per pair that wants `newtgt`, the path from path32_ws.
__global__ void __launch_bounds__(256)
dtw_fused_align_kernel(const double *__restrict__ feats, const DtwPair *__restrict__ pairs, int D, int Smax, int Tmax,
                       const int32_t *__restrict__ path32_ws) {
  const DtwPair P = pairs[blockIdx.x];
  if (!P.newtgt || P.T == 0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int SmaxE = (Smax + 1) & ~1;
  int32_t *path32 = reinterpret_cast<int32_t *>(smem_raw);            // [Tmax]
  int32_t *owner = path32 + Tmax;                                     // [SmaxE]
  int32_t *holes = owner + SmaxE;                                     // [SmaxE]
  for (int t = threadIdx.x; t < P.T; t += 256) path32[t] = path32_ws[P.path32_off + t];
  __syncthreads();
  dtw_align_post(P, feats + P.seq_off, D, path32, owner, holes);
}

// descriptors of a call: pinned host slot -> device (16 bytes per thread)
__global__ void __launch_bounds__(256) dtw_desc_copy_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n16) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n16) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// Dynamic LDS of the two fused kernels; the caller takes the observation + recurrence path when either exceeds the budget
// (sequences beyond ~9.7k frames: the forward kernel keeps the boundary costs of a strip, 16 bytes per column, in LDS).
static inline size_t dtw_fused_lds_forward(int Tmax) {
  return (size_t)4 * VCMI_FUSED_OUTBOX + (size_t)2 * kFusedRows * 8 + ((size_t)Tmax + 1) * 16;
}
static inline size_t dtw_fused_lds_finish(int Smax, int Tmax) {      // dtw_fused_align_kernel: path, owner, holes
  const size_t SmaxE = (size_t)((Smax + 1) & ~1);
  return (size_t)Tmax * 4 + SmaxE * 8;
}
bool dtw_fused_fits(int Smax, int Tmax) {
  return dtw_fused_lds_forward(Tmax) <= kLdsLimit && dtw_fused_lds_finish(Smax, Tmax) <= kLdsLimit;
}

// Row length the fused forward kernel works on.  D = 41 -- order-40 mel-cepstra WITH c0, what the reference's own pipeline
// aligns (bin/mcep.jl:12 --order=40, bin/align.jl:42-45 -> src/align.jl:45 -> src/dtw.jl:33-35) -- has its own loop that
// reads the 41-double rows as they lie in memory (no padded copy); every other D is padded up to the next instantiation.
static int dtw_fused_row(int D) { return D == 41 ? 41 : dtw_dmax(D); }

// Fused path of dtw_run (see dtw_fused_kernel): the job list (dtw_fused_plan), workspaces, the one descriptor upload, the
// forward launch and the backward / align launch.
int dtw_run_fused(const double *feats, std::vector<DtwPair> &pairs, int D, int bstep, DtwScratch &sc, hipStream_t st, int Smax,
                  int Tmax) {
  const int n = (int)pairs.size();
  const int dmax = dtw_fused_row(D);
  int slots = 512;
  {
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    slots = 2 * cus;                              // two workgroups per CU (set by the registers)
  }
  const DtwFusedPlan plan = dtw_fused_plan(pairs, dmax, slots, !debug_flag(kDbgDtwNoSegments), debug_flag(kDbgDtwTwoSegments),
                                           debug_flag(kDbgDtwWholeFirst));
  const std::vector<DtwStrip> &strips = plan.strips;
  const std::vector<int> &job_first = plan.job_first;
  const unsigned ngroups = (unsigned)job_first.size();
  if (strips.empty()) return VCMI_OK;
  VCMI_TRY(sc.fcodes.reserve(plan.ncodes));
  VCMI_TRY(sc.clast.reserve(plan.nclast));
  VCMI_TRY(sc.path32.reserve(std::max<size_t>(plan.npath, 1)));
  VCMI_TRY(sc.bnd.reserve(std::max<size_t>(plan.nbnd, 1)));
  const int nflags = plan.nflags;
  if ((size_t)nflags > sc.flags.n) {
    VCMI_TRY(sc.flags.reserve(std::max<size_t>((size_t)nflags, 1024)));
    VCMI_HIP(hipMemsetAsync(sc.flags.p, 0, sc.flags.n * sizeof(int), st));
    sc.epoch = 0;
  }
  const int epoch = ++sc.epoch;
  // one upload for everything the kernels read: [pairs | strips | first descriptor of every job, ticket counter = 0]
  const size_t o_strips = ((size_t)n * sizeof(DtwPair) + 255) & ~(size_t)255;
  const size_t o_jobs = (o_strips + strips.size() * sizeof(DtwStrip) + 255) & ~(size_t)255;
  const size_t desc_bytes = (o_jobs + (job_first.size() + 1) * sizeof(int) + 15) & ~(size_t)15;
  VCMI_TRY(sc.ddesc.reserve(desc_bytes));
  unsigned char *descp = sc.ddesc.p;
  {
    unsigned char *pinned = nullptr;
    hipEvent_t copied = nullptr;
    VCMI_TRY(sc.stage_raw(desc_bytes, &pinned, &copied));
    memcpy(pinned, pairs.data(), (size_t)n * sizeof(DtwPair));
    memcpy(pinned + o_strips, strips.data(), strips.size() * sizeof(DtwStrip));
    memcpy(pinned + o_jobs, job_first.data(), job_first.size() * sizeof(int));
    memset(pinned + o_jobs + job_first.size() * sizeof(int), 0, sizeof(int));
    // a copy KERNEL reading the pinned slot, not hipMemcpyAsync: the copy engine's hand-over to the compute queue left the
    // GPU idle for ~36 us between consecutive calls (kernel trace); a kernel on the same queue starts within a few us
    hipLaunchKernelGGL(dtw_desc_copy_kernel, dim3((unsigned)((desc_bytes / 16 + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const uint4 *>(pinned), reinterpret_cast<uint4 *>(sc.ddesc.p), desc_bytes / 16);
    VCMI_HIP(hipEventRecord(copied, st));
  }
  const DtwPair *dpairs = reinterpret_cast<const DtwPair *>(descp);
  const DtwStrip *dstrips = reinterpret_cast<const DtwStrip *>(descp + o_strips);
  int *djobs = reinterpret_cast<int *>(descp + o_jobs);
  int *ticket = djobs + job_first.size();
  const bool padded = (D != dmax);
  if (padded) {
    VCMI_TRY(sc.spad.reserve(plan.padn));
    dtw_launch_pad(feats, dpairs, n, D, dmax, sc.spad.p, st);
  }
  const double *base = padded ? sc.spad.p : feats;
  const size_t shf = dtw_fused_lds_forward(Tmax);
  if (shf > kLdsLimit) return fail(VCMI_ERR_ARG, "DTW: sequence of %d frames exceeds the supported length", Tmax);
#define VCMI_FUSED_LAUNCH(DM, STP)                                                                                    \
  do {                                                                                                                \
    if ((int)ngroups > slots && DM <= 41 && !debug_flag(kDbgDtwGridOrder)) { /* more jobs than slots: ticket-drawn */ \
      auto kernp = dtw_fused_persistent_kernel<DM, STP>;                                                              \
      VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernp), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                   (int)shf));                                                                        \
      hipLaunchKernelGGL(kernp, dim3((unsigned)slots), dim3(kFusedThreads), shf, st, base, (int)padded, dpairs,  \
                         dstrips, sc.fcodes.p, sc.bnd.p, sc.clast.p, sc.flags.p, epoch, djobs, (int)ngroups, \
                         ticket);                                                                                     \
    } else {                                                                                                          \
      auto kern = dtw_fused_kernel<DM, STP>;                                                                          \
      VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,  \
                                   (int)shf));                                                                        \
      hipLaunchKernelGGL(kern, dim3(ngroups), dim3(kFusedThreads), shf, st, base, (int)padded, dpairs,           \
                         dstrips, sc.fcodes.p, sc.bnd.p, sc.clast.p, sc.flags.p, epoch, djobs);             \
    }                                                                                                                 \
  } while (0)
#define VCMI_FUSED_CASE(DM) \
  case DM: if (bstep == 1) VCMI_FUSED_LAUNCH(DM, 1); else VCMI_FUSED_LAUNCH(DM, 2); break;
  switch (dmax) {
    VCMI_FUSED_CASE(8) VCMI_FUSED_CASE(16) VCMI_FUSED_CASE(24) VCMI_FUSED_CASE(32) VCMI_FUSED_CASE(40) VCMI_FUSED_CASE(41)
    VCMI_FUSED_CASE(48)
  }
#undef VCMI_FUSED_CASE
#undef VCMI_FUSED_LAUNCH
  VCMI_HIP(hipGetLastError());
  // backward (a wave per pair), then align() for the pairs that want it
  hipLaunchKernelGGL(dtw_fused_backward_kernel, dim3((unsigned)n), dim3(64), (size_t)Tmax * 4, st, dpairs, sc.fcodes.p, sc.clast.p,
                     sc.path32.p);
  if (plan.any_align) {
    const size_t shb = dtw_fused_lds_finish(Smax, Tmax);
    if (shb > kLdsLimit) return fail(VCMI_ERR_ARG, "DTW: template of %d frames exceeds the supported length", Smax);
    auto kern = dtw_fused_align_kernel;
    VCMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shb));
    hipLaunchKernelGGL(kern, dim3(n), dim3(256), shb, st, feats, dpairs, D, Smax, Tmax, sc.path32.p);
  }
  VCMI_HIP(hipGetLastError());
  VCMI_HIP(hipEventRecord(sc.last_use, st));
#ifdef VCMI_DTW_PROF
  {
    unsigned long long h[8], z[8] = {0};
    (void)hipStreamSynchronize(st);
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(dtw_prof), sizeof(h));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(dtw_prof), z, sizeof(z));
    if (h[3])
      fprintf(stderr, "dtw_prof: %llu jobs (nseg %d); cycles per job: prologue %.0f (of which flag wait %.0f), column loop %.0f, epilogue %.0f\n",
              h[3], plan.nseg, (double)h[0] / h[3], (double)h[4] / h[3], (double)h[1] / h[3], (double)h[2] / h[3]);
  }
#endif
  return VCMI_OK;
}

}  // namespace vcmi
