// gmmmap_group.hip -- the stable counting sort of frames by an integer key (grouping.hpp): fvconvert's and predict's grouping
// by nearest source mean (key kernels, the two-launch sort, launch_grouping) and the scan + scatter pair that the E-step's
// hard path (estep.hip) launches behind its gate.
#include "grouping.hpp"
#include "gmmmap_handle.hpp"
#include "gmmmap_rows.hpp"
#include "bf16_split.hpp"

#include <algorithm>
#include <cmath>

namespace vcmi {

// ------------------------------------------------------------------------------------------------
// Grouping of the frames before fvconvert (gmmmap_mfma_kernel MODE 0 with perm / gkey, gmmmap.hip).
// The pruning of the convert kernel works per 16-frame tile: a regression is skipped when NONE of the tile's frames gives the
// mixture a posterior above e^-prune.  Frames that arrive in an order unrelated to their mixtures (the benchmark draws them
// independently: ~14 of 64 mixtures own a frame of a tile, and the loop meets ~24 before its running maximum is tight) make
// that union large; the same frames grouped by mixture leave one or two.  The grouping does not have to be right -- any
// permutation gives the same y, frame by frame -- only cheap and mostly right: the NEAREST SOURCE MEAN (Euclidean), one
// small MFMA product per tile ([-2 mu | |mu|^2] x [x ; 1], 44 MFMAs per 16 frames at D = 40, M = 64 against 2400 for the
// conversion).  A STABLE counting sort (round 4; the first version ranked with LDS / global atomics, which left the order
// inside a group -- hence the tiles, the rotated mixture order of a boundary workgroup and the last bit of a frame shared by
// several mixtures -- to the scheduler) in TWO launches: keys + a histogram per chunk of 1024 frames and per super-chunk of
// ~sqrt(nchunks) chunks (gmmmap_group_key16_kernel / gmmmap_group_key_kernel), and the scatter, every workgroup of which sums
// the few histogram rows in front of its chunk itself (gmmmap_group_place_kernel).  It used to be three: a prefix over
// (group, chunk) stood between them (gmmmap_group_scan_kernel) only to hand every scatter workgroup that sum -- a launch, its
// drain and its ramp on a path of four dependent kernels.  The E-step's hard path (estep.hip), whose launches are gated by a
// device word, still runs that scan and gmmmap_group_scatter_kernel.  The scatter also leaves gbase[0 .. M], the first
// sorted position of every group: the screen kernels take their groups from it instead of a key per frame.
// gfrag[mt][ks][lane]: A-operand fragments, rows = mixtures 16 mt + (lane & 15), k = 4 ks + (lane >> 4); the last k-step
// carries |mu|^2 (rows >= M: 1e300, never the minimum).
// ------------------------------------------------------------------------------------------------
// keys + one histogram per CHUNK of 1024 consecutive frames (chunkhist[c][m]); a workgroup walks chunks blockIdx.x,
// blockIdx.x + gridDim.x, ... with the operand fragments staged once.  The counts are integers: whatever order the LDS
// atomics arrive in, the histogram is the same.  superhist[c >> super_shift][m] (zero on entry: launch_grouping) receives
// the chunk histograms' sums by vector atomic adds to global memory, integers again.
template <int DP>
__global__ void __launch_bounds__(256)
gmmmap_group_key_kernel(const double *__restrict__ gfrag, int M, int D, const double *__restrict__ X, int64_t ldx, int64_t T,
                        int *__restrict__ key, int *__restrict__ chunkhist, int *__restrict__ superhist, int super_shift) {
  // KS: the k-steps the key LOOKS AT -- the first 24 dimensions at most (kGroupKeyDims).  The key only has to be cheap and
  // mostly right, and the distance over 24 of 40 dimensions picks the same groups (CPU simulation of the kernel's rule, 6e4
  // frames: regressions evaluated 0.0168 / 0.0168 on the SURVEY 8d model, 0.6765 / 0.6760 on the reference's trained model,
  // 0.0351 / 0.0341 on the broad synthetic one; 16 dimensions: 0.0168 / 0.680 / 0.081) for 28 instead of 44 MFMAs per tile.
  constexpr int KS = (DP / 4 < kGroupKeyDims / 4) ? DP / 4 : kGroupKeyDims / 4, KS1 = KS + 1;
  extern __shared__ double gsm[];
  const int MT = (M + 15) / 16, nfrag = MT * KS1 * 64;
  int *hist = reinterpret_cast<int *>(gsm + nfrag);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lcol = lane & 15, lgrp = lane >> 4;
  for (int e = tid; e < nfrag; e += 256) gsm[e] = gfrag[e];
  const double one = (lgrp == 0) ? 1.0 : 0.0;
  const int64_t nchunks = (T + kGroupChunk - 1) / kGroupChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    for (int m = tid; m < M; m += 256) hist[m] = 0;
    __syncthreads();
    for (int i = 0; i < kGroupChunk / 64; ++i) {
      const int64_t fr = c * kGroupChunk + 16 * (4 * i + wave) + lcol;
      if (fr - lcol >= T) break;                                    // (wave-uniform)
      double xb[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int k = 4 * ks + lgrp;
        xb[ks] = (fr < T && k < D) ? X[fr * ldx + k] : 0.0;
      }
      double best = INFINITY;
      int bm = 0;
      for (int mt = 0; mt < MT; ++mt) {
        const double *A = gsm + (size_t)mt * KS1 * 64 + lane;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[ks * 64], xb[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[KS * 64], one, acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (acc[r] < best) {
            best = acc[r];
            bm = 16 * mt + 4 * r + lgrp;
          }
      }
#pragma unroll
      for (int sh = 16; sh < 64; sh <<= 1) {
        const double ov = __shfl_xor(best, sh);
        const int om = __shfl_xor(bm, sh);
        if (ov < best || (ov == best && om < bm)) {
          best = ov;
          bm = om;
        }
      }
      if (lgrp == 0 && fr < T) {
        bm = bm < M ? bm : 0;
        key[fr] = bm;
        atomicAdd(&hist[bm], 1);
      }
    }
    __syncthreads();
    for (int m = tid; m < M; m += 256) {
      const int h = hist[m];
      chunkhist[c * M + m] = h;
      if (h) atomicAdd(&superhist[(c >> super_shift) * M + m], h);   // (integers: the sum does not depend on the order of arrival)
    }
    __syncthreads();
  }
}

// The same keys on the BF16 matrix pipe (round 5).  The key only has to be mostly right, and the FP64 products were half of the
// kernel's time (28 MFMAs of 64 cycles per tile beside a read of x that is bound by HBM): -2 mu and x are split into bf16
// hi + lo (gmmmap_screen.hpp: split_bf16; products to ~2^-16 relative) and the distances over the first 24 dimensions are three
// v_mfma_f32_16x16x32_bf16 per 16 mixtures (slot j of lane group g <-> feature 4 j + g: the lane's own FP64 operand), |mu|^2
// in the accumulator's initial value.  gfrag16[mt]: 64 x 16 bytes of hi, 64 x 16 bytes of lo, 4 x 4 floats of |mu|^2 (lane
// group g of the result holds rows 4 g .. 4 g + 3; rows >= M: 1e30).  Deterministic like the FP64 kernel; a frame between
// two means may get the other key, which costs a regression, never a result.
template <int DP>
__global__ void __launch_bounds__(256)
gmmmap_group_key16_kernel(const double *__restrict__ gfrag16, int M, int D, const double *__restrict__ X, int64_t ldx, int64_t T,
                          int *__restrict__ key, int *__restrict__ chunkhist, int *__restrict__ superhist, int super_shift) {
  constexpr int KS = (DP / 4 < kGroupKeyDims / 4) ? DP / 4 : kGroupKeyDims / 4;
  static_assert(KS <= 8, "one K = 32 instruction per term");
  extern __shared__ double gsm[];
  const int MT = (M + 15) / 16, nd = MT * (kKey16TileBytes / 8);
  int *hist = reinterpret_cast<int *>(gsm + nd);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lcol = lane & 15, lgrp = lane >> 4;
  for (int e = tid; e < nd; e += 256) gsm[e] = gfrag16[e];
  const int64_t nchunks = (T + kGroupChunk - 1) / kGroupChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    for (int m = tid; m < M; m += 256) hist[m] = 0;
    __syncthreads();
    // two frame tiles per pass: both tiles' rows are requested before either is used (the kernel is a chain of exposed load
    // latencies: 16 passes per wave and chunk, each waiting for its rows -- round 6)
    for (int i = 0; i < kGroupChunk / 64; i += 2) {
      const int64_t fr0 = c * kGroupChunk + 16 * (4 * i + wave) + lcol;
      if (fr0 - lcol >= T) break;                                   // (wave-uniform)
      double xv[2][KS];
      const bool klines = rows_as_lines(X, ldx, D, DP);             // (whole lines for the first 16 features: load_frame_row)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int64_t fr = fr0 + 64 * u;
        load_frame_row<KS>(X + (fr < T ? fr : T - 1) * ldx, true, klines, D, lgrp, xv[u]);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int64_t fr = fr0 + 64 * u;
        if (fr - lcol >= T) break;                                  // (wave-uniform: the second tile of the pass lies beyond T)
        u32x4_t bh = {0u, 0u, 0u, 0u}, bl = {0u, 0u, 0u, 0u};
        {
          unsigned short h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, l[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const int k = 4 * ks + lgrp;
            const double x = (fr < T && k < D) ? xv[u][ks] : 0.0;
            split_bf16(x, h[ks], l[ks]);
          }
#pragma unroll
          for (int w2 = 0; w2 < 4; ++w2) {
            bh[w2] = (unsigned)h[2 * w2] | ((unsigned)h[2 * w2 + 1] << 16);
            bl[w2] = (unsigned)l[2 * w2] | ((unsigned)l[2 * w2 + 1] << 16);
          }
        }
        float best = INFINITY;
        int bm = 0;
        for (int mt = 0; mt < MT; ++mt) {
          const char *tb = reinterpret_cast<const char *>(gsm) + (size_t)mt * kKey16TileBytes;
          const u32x4_t aph = *reinterpret_cast<const u32x4_t *>(tb + 16 * lane), apl = *reinterpret_cast<const u32x4_t *>(tb + 1024 + 16 * lane);
          f32x4_t acc = *reinterpret_cast<const f32x4_t *>(tb + 2048 + 16 * lgrp);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, aph), __builtin_bit_cast(bf16x8_t, bh), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, aph), __builtin_bit_cast(bf16x8_t, bl), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, apl), __builtin_bit_cast(bf16x8_t, bh), acc, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (acc[r] < best) {
              best = acc[r];
              bm = 16 * mt + 4 * lgrp + r;
            }
        }
#pragma unroll
        for (int sh = 16; sh < 64; sh <<= 1) {
          const float ov = __shfl_xor(best, sh);
          const int om = __shfl_xor(bm, sh);
          if (ov < best || (ov == best && om < bm)) {
            best = ov;
            bm = om;
          }
        }
        if (lgrp == 0 && fr < T) {
          bm = bm < M ? bm : 0;
          key[fr] = bm;
          atomicAdd(&hist[bm], 1);
        }
      }
    }
    __syncthreads();
    for (int m = tid; m < M; m += 256) {
      const int h = hist[m];
      chunkhist[c * M + m] = h;
      if (h) atomicAdd(&superhist[(c >> super_shift) * M + m], h);   // (integers: the sum does not depend on the order of arrival)
    }
    __syncthreads();
  }
}

// One workgroup per group m: chunkhist[c][m] -> its exclusive prefix over the chunks (in place) and total[m].
__global__ void __launch_bounds__(256)
gmmmap_group_scan_kernel(int *__restrict__ chunkhist, int64_t nchunks, int M, int *__restrict__ total, const int64_t *__restrict__ gate) {
  if (gate && *gate == 0) return;
  __shared__ int wtot[4];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t per = (nchunks + 255) / 256, lo = std::min<int64_t>(nchunks, tid * per), hi = std::min<int64_t>(nchunks, lo + per);
  int sum = 0;
  for (int64_t c = lo; c < hi; ++c) sum += chunkhist[c * M + m];
  // exclusive prefix of the 256 stretch sums: shuffles within a wave, the four wave totals through LDS (integers: any order
  // gives the same numbers; one thread walking 256 LDS entries took 7 of the kernel's 10 us)
  int inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wtot[w];
  if (tid == 255) total[m] = base + inc;
  int run = base + inc - sum;
  for (int64_t c = lo; c < hi; ++c) {
    const int v = chunkhist[c * M + m];
    chunkhist[c * M + m] = run;
    run += v;
  }
}

// perm: frames in group order, and inside a group in FRAME order (a stable counting sort: the permutation, hence every tile
// of the convert kernel and every sum it forms, is a function of the data alone -- repeat runs are bit-identical).  One
// workgroup per chunk; position = sum of the smaller groups' totals + the group's frames in earlier chunks + those in earlier
// 64-frame rows of this chunk + those on lower lanes of the row.  The two kernels below differ in where the first two terms
// come from; the rest is scatter_chunk().
// base[m] (LDS): the groups' totals -> their exclusive prefix (wave 0: a lane sums its stretch, the lanes' sums are scanned by
// shuffles; one thread walking the totals took 10 us per workgroup at 128 groups).  Barriers around it are the caller's.
__device__ __forceinline__ void group_bases_from_totals(int *base, int M, int lane) {
  const int per = (M + 63) / 64, lo = lane * per, hi = (lo + per < M) ? lo + per : M;
  int s = 0;
  for (int m = lo; m < hi; ++m) s += base[m];
  int incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  int run = incl - s;
  for (int m = lo; m < hi; ++m) {
    const int v = base[m];
    base[m] = run;
    run += v;
  }
}
// base[m] (LDS, visible): first position of group m's frames of this chunk; rowcnt: [16][M] zeros (visible)
__device__ __forceinline__ void scatter_chunk(const int *__restrict__ key, int64_t T, int M, int64_t f0, const int *base, int *rowcnt,
                                              int *__restrict__ perm) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int k[4], rank[4];
  const int nbits = 32 - __builtin_clz((unsigned)(M > 1 ? M - 1 : 1));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = wave + 4 * i;                                   // row of 64 consecutive frames
    const int64_t fr = f0 + 64 * r + lane;
    k[i] = fr < T ? key[fr] : -1;
    // the lanes of the row that hold the same key, by one ballot per key BIT (log2 M turns whatever the number of distinct
    // keys: unsorted keys of 128 groups put ~40 distinct ones into a row, one turn each in the first version)
    unsigned long long eq = __builtin_amdgcn_ballot_w64(k[i] >= 0);
    for (int b = 0; b < nbits; ++b) {
      const bool bit = (k[i] >> b) & 1;
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(bit);
      eq &= bit ? bal : ~bal;
    }
    rank[i] = __builtin_amdgcn_mbcnt_hi((unsigned)(eq >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)eq, 0));
    if (k[i] >= 0 && rank[i] == 0) rowcnt[r * M + k[i]] = __builtin_popcountll(eq);
  }
  __syncthreads();
  for (int m = tid; m < M; m += 256) {
    int run = 0;
    for (int r = 0; r < 16; ++r) {
      const int v = rowcnt[r * M + m];
      rowcnt[r * M + m] = run;
      run += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = wave + 4 * i;
    const int64_t fr = f0 + 64 * r + lane;
    if (k[i] >= 0) {
      const int64_t pos = (int64_t)base[k[i]] + rowcnt[r * M + k[i]] + rank[i];
      if (pos < T) perm[pos] = (int)fr;                            // (always, with consistent histograms: never a store past perm)
    }
  }
}

// After gmmmap_group_scan_kernel: chunkhist holds the prefix over the chunks, total[] the groups' sizes (the E-step's hard path).
__global__ void __launch_bounds__(256)
gmmmap_group_scatter_kernel(const int *__restrict__ key, int64_t T, int M, const int *__restrict__ chunkhist,
                            const int *__restrict__ total, int *__restrict__ perm, const int64_t *__restrict__ gate) {
  if (gate && *gate == 0) return;
  extern __shared__ int lsm[];             // [M] group bases, then [16][M] row counts -> row bases
  int *base = lsm, *rowcnt = lsm + M;
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  for (int m = tid; m < M; m += 256) base[m] = total[m];
  for (int e = tid; e < 16 * M; e += 256) rowcnt[e] = 0;
  __syncthreads();
  if (tid < 64) group_bases_from_totals(base, M, tid);
  __syncthreads();
  for (int m = tid; m < M; m += 256) base[m] += chunkhist[c * M + m];
  __syncthreads();
  scatter_chunk(key, T, M, c * kGroupChunk, base, rowcnt, perm);
}

// The same scatter WITHOUT a scan launch in front of it (fvconvert, predict): the key kernel has also summed its chunk
// histograms into one row per SUPER-CHUNK of 2^super_shift chunks (superhist[s][m], nsuper rows), and workgroup c forms what it
// needs from those by itself: the groups' totals = the sum of all super-chunk rows, the group's frames in earlier chunks = the
// super-chunk rows before its own + the chunk rows of its own super-chunk before c.  Both are reads of rows that the key
// kernel -- an earlier launch -- has finished: no workgroup waits for another one.  2^super_shift ~ sqrt(nchunks) (32 at 10^6
// frames: at most 31 + 31 coalesced rows of M ints per workgroup).
// Workgroup 0 also leaves gbase[0 .. M] (the exclusive prefix of the totals, gbase[M] = T): sorted position p belongs to group
// m exactly when gbase[m] <= p < gbase[m + 1], which is all the screen kernels want to know (gmmmap_screen.hpp).
// clear[0 .. nclear): the OTHER super-chunk table, zeroed here for the next call (launch_grouping explains why that is safe).
__global__ void __launch_bounds__(256)
gmmmap_group_place_kernel(const int *__restrict__ key, int64_t T, int M, const int *__restrict__ chunkhist,
                          const int *__restrict__ superhist, int nsuper, int super_shift, int *__restrict__ clear, int64_t nclear,
                          int *__restrict__ gbase, int *__restrict__ perm) {
  extern __shared__ int lsm[];             // [M] totals -> group bases, [16][M] row counts -> row bases, [M] frames in earlier chunks
  int *base = lsm, *rowcnt = lsm + M, *before = lsm + 17 * M;
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  for (int64_t e = c * 256 + tid; e < nclear; e += (int64_t)gridDim.x * 256) clear[e] = 0;
  for (int m = tid; m < M; m += 256) {
    base[m] = 0;
    before[m] = 0;
  }
  for (int e = tid; e < 16 * M; e += 256) rowcnt[e] = 0;
  __syncthreads();
  {
    // up to 256 groups: thread <-> (row slot, group), `slots` rows in flight; more: thread <-> group, row after row
    const int slots = M <= 256 ? 256 / M : 1, slot = M <= 256 ? tid / M : 0;
    const int own = (int)(c >> super_shift);
    const int64_t c_lo = (int64_t)own << super_shift;
    if (slot < slots) {
      for (int m = M <= 256 ? tid % M : tid; m < M; m += 256) {
        int tot = 0, bef = 0;
#pragma unroll 4
        for (int s = slot; s < nsuper; s += slots) {
          const int v = superhist[(int64_t)s * M + m];
          tot += v;
          bef += s < own ? v : 0;
        }
#pragma unroll 4
        for (int64_t cc = c_lo + slot; cc < c; cc += slots) bef += chunkhist[cc * M + m];
        atomicAdd(&base[m], tot);                                  // (integers: any order gives the same sums)
        atomicAdd(&before[m], bef);
      }
    }
  }
  __syncthreads();
  if (tid < 64) group_bases_from_totals(base, M, tid);
  __syncthreads();
  if (c == 0)
    for (int m = tid; m <= M; m += 256) gbase[m] = m < M ? base[m] : (int)T;
  __syncthreads();
  for (int m = tid; m < M; m += 256) base[m] += before[m];
  __syncthreads();
  scatter_chunk(key, T, M, c * kGroupChunk, base, rowcnt, perm);
}

// calls of fewer frames are not grouped (the sort's two launches do not pay: tools/small_T_sweep.py)
static constexpr int64_t kSortMinFrames = 8192;

// The two grouping kernels (keys + chunk and super-chunk histograms, stable scatter) on g's scratch: *perm = frames in group
// order, *gbase = first sorted position of every group (M + 1 ints), *key = group of every frame.  The caller brackets its use
// of them with g->grp_order.enter / leave.
static size_t group_key_shmem(const vcmi_gmmmap *g, bool fp64) {
  return (fp64 ? group_key_doubles(g->DP, g->M) : group_key16_doubles(g->M)) * sizeof(double) + (size_t)g->M * sizeof(int);
}
static bool group_key_fp64(const vcmi_gmmmap *g) { return debug_flag(kDbgGroupKeyFp64) || !g->gfrag16.p; }
bool can_group(const vcmi_gmmmap *g, int64_t T) {
  return T >= kSortMinFrames && T < ((int64_t)1 << 31) && g->M >= 4 && g->gfrag.p && group_key_shmem(g, group_key_fp64(g)) <= 64 * 1024;
}
// chunks per super-chunk, as a shift: the power of two from 32 on that reaches sqrt(nchunks) -- a scatter workgroup reads
// nsuper + 2^shift rows at most, so the two terms are kept alike
static int group_super_shift(int64_t nchunks) {
  int sh = 5;
  while (((int64_t)1 << (2 * sh)) < nchunks) ++sh;
  return sh;
}
int launch_grouping(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, hipStream_t st, int **key_out, int **perm_out,
                    int **gbase_out) {
  const bool fp64 = group_key_fp64(g);
  const size_t gshmem = group_key_shmem(g, fp64);
  const int64_t nchunks = (T + kGroupChunk - 1) / kGroupChunk;
  const int sshift = group_super_shift(nchunks);
  const int64_t nsuper = (nchunks + ((int64_t)1 << sshift) - 1) >> sshift;
  const size_t sneed = (size_t)nsuper * g->M;
  VCMI_TRY(g->grp.reserve((size_t)2 * T + (size_t)nchunks * g->M + (size_t)g->M + 1));
  if (sneed > g->grp_super_stride) {
    g->grp_super_ok = false;
    g->grp_super_stride = 0;
    VCMI_TRY(g->grp_super.alloc(2 * sneed));
    g->grp_super_stride = sneed;
  }
  VCMI_TRY(g->grp_order.enter(st));
  // The super-chunk table that the key kernel adds into must be all zero when it starts, without a memset in every call: there
  // are two, call n uses table n & 1 and its scatter kernel zeroes what call n - 1 left in the other one, for call n + 1.  That
  // is safe because everything that touches the tables is ordered: within a call the key kernel, the scatter kernel and the
  // next call's key kernel follow each other on the stream (or, on another stream, behind grp_order's event, which the
  // caller records after its last kernel) -- the table being cleared was last read by the scatter kernel of call n - 1, which
  // has finished, and is next written by the key kernel of call n + 1, which has not begun.  Only a buffer that is new, or a
  // call that returned between its launches, leaves them in an unknown state: both are then zeroed here, once.
  // A call that is being CAPTURED into a graph runs again and again with the table of this one visit: it zeroes both tables
  // itself, inside the graph, and leaves the state unknown for the next call outside it.
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess) {
    (void)hipGetLastError();
    cap = hipStreamCaptureStatusNone;
  }
  const bool captured = cap != hipStreamCaptureStatusNone;
  if (!g->grp_super_ok || captured) {
    VCMI_HIP(hipMemsetAsync(g->grp_super.p, 0, 2 * g->grp_super_stride * sizeof(int), st));
    g->grp_super_used[0] = g->grp_super_used[1] = 0;
  }
  g->grp_super_ok = false;
  const unsigned cur = g->grp_calls & 1u, oth = cur ^ 1u;
  int *key = g->grp.p, *perm = key + T, *chunkhist = perm + T, *gbase = chunkhist + nchunks * g->M;
  int *superhist = g->grp_super.p + cur * g->grp_super_stride, *superclear = g->grp_super.p + oth * g->grp_super_stride;
  const unsigned kgrid = (unsigned)std::min<int64_t>(nchunks, (int64_t)g->cus * 4);
  switch (g->DP) {
#define VCMI_CASE(DPV) \
  case DPV: \
    if (fp64) hipLaunchKernelGGL(gmmmap_group_key_kernel<DPV>, dim3(kgrid), dim3(256), gshmem, st, g->gfrag.p, g->M, g->D, dX, ldx, T, key, chunkhist, superhist, sshift); \
    else hipLaunchKernelGGL(gmmmap_group_key16_kernel<DPV>, dim3(kgrid), dim3(256), gshmem, st, g->gfrag16.p, g->M, g->D, dX, ldx, T, key, chunkhist, superhist, sshift); \
    break;
    VCMI_TILE_DIMS(VCMI_CASE)
#undef VCMI_CASE
    default: return fail(VCMI_ERR_ARG, "no MFMA instantiation for padded dimension %d", g->DP);
  }
  VCMI_HIP(hipGetLastError());
  hipLaunchKernelGGL(gmmmap_group_place_kernel, dim3((unsigned)nchunks), dim3(256), (size_t)18 * g->M * sizeof(int), st,
                     key, T, g->M, chunkhist, superhist, (int)nsuper, sshift, superclear, (int64_t)g->grp_super_used[oth], gbase, perm);
  VCMI_HIP(hipGetLastError());
  if (!captured) {
    g->grp_super_used[cur] = sneed;
    g->grp_super_used[oth] = 0;
    ++g->grp_calls;
    g->grp_super_ok = true;
  }
  *key_out = key;
  *perm_out = perm;
  *gbase_out = gbase;
  return VCMI_OK;
}

}  // namespace vcmi
