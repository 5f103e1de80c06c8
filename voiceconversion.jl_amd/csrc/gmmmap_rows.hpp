// gmmmap_rows.hpp -- what the tile kernel (gmmmap.hip), the screen kernels (gmmmap_screen.hpp) and the grouping's key kernel
// (gmmmap_group.hip) share: sums and transposes across the four lane groups of an MFMA result column, and the rows of x and y
// as whole 128-byte lines.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace vcmi {

typedef double d4 __attribute__((ext_vector_type(4)));

// q[lane] -> the sum over the four lanes {lane % 16 + 16 g} (the lane groups of an MFMA result column), in every lane.
// v_permlane16_swap / v_permlane32_swap (gfx950) exchange 16-lane rows / wave halves between two registers, so each level is
// two moves, two swaps per 32-bit half and one add -- no LDS round trip (__shfl_xor compiles to ds_bpermute_b32 pairs with an
// s_waitcnt each).  Same pairs added in the same association as q += shfl_xor(q, 16); q += shfl_xor(q, 32): bit-identical.
__device__ __forceinline__ double sum_lane_groups(double q) {
  unsigned lo = __double2loint(q), hi = __double2hiint(q);
  auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const double x = __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
  lo = __double2loint(x);
  hi = __double2hiint(x);
  auto c = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  auto d = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double(d[0], c[0]) + __hiloint2double(d[1], c[1]);
}

// Two columns' worth at once: q0[lane], q1[lane] -> in the EVEN lane groups the lane-group sum of q0, in the ODD ones that of
// q1.  The first exchange swaps 16-lane rows between the two registers themselves (no copies): six moves / swaps and two adds
// instead of the sixteen and four of two sum_lane_groups calls -- and every VALU instruction of a wave, FP64 or not, waits
// for the FP64 MFMAs of the SIMD's other waves.  Association: (q_g + q_g^1) + (the other pair), as in sum_lane_groups.
__device__ __forceinline__ double sum_lane_groups_pair(double q0, double q1) {
  const unsigned l0 = __double2loint(q0), h0 = __double2hiint(q0), l1 = __double2loint(q1), h1 = __double2hiint(q1);
  auto a = __builtin_amdgcn_permlane16_swap(l0, l1, false, false);     // {rows (q0 r0, q1 r0, q0 r2, q1 r2), rows (q0 r1, q1 r1, q0 r3, q1 r3)}
  auto b = __builtin_amdgcn_permlane16_swap(h0, h1, false, false);
  const double x = __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
  const unsigned lo = __double2loint(x), hi = __double2hiint(x);
  auto c = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  auto d = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double(d[0], c[0]) + __hiloint2double(d[1], c[1]);
}
// v (selected layout: tile 0's value in the even lane groups, tile 1's in the odd ones) -> {tile 0's, tile 1's} in every lane
__device__ __forceinline__ void unpair_lane_groups(double v, double &v0, double &v1) {
  const unsigned lo = __double2loint(v), hi = __double2hiint(v);
  auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  v0 = __hiloint2double(b[0], a[0]);
  v1 = __hiloint2double(b[1], a[1]);
}

// ------------------------------------------------------------------------------------------------
// Rows of x and y as whole 128-byte lines (round 6).  The MFMA operand / result layout gives lane group g of a frame's column the
// features 4 j + g (slot j = k-step j): a load or store instruction then touches 32 bytes of each of its 16 frames, and the
// pieces cost ~8 % of the screened conversion's step (profiles/r06_ab).  Where the rows are 16-byte aligned and unpadded, lane
// group g moves features 16 b + 4 g .. + 3 instead -- 32 contiguous bytes per lane, a line per frame and block of four slots --
// and a 4 x 4 transpose across the lane groups (two exchange stages: wave halves with v_permlane32_swap, then 16-lane rows with
// v_permlane16_swap; an involution) converts between the two: (slot j, group g) <-> (slot g, group j).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void transpose_lane_groups4(double &e0, double &e1, double &e2, double &e3) {
  unsigned lo[4] = {(unsigned)__double2loint(e0), (unsigned)__double2loint(e1), (unsigned)__double2loint(e2), (unsigned)__double2loint(e3)};
  unsigned hi[4] = {(unsigned)__double2hiint(e0), (unsigned)__double2hiint(e1), (unsigned)__double2hiint(e2), (unsigned)__double2hiint(e3)};
#pragma unroll
  for (int j = 0; j < 2; ++j) {                              // lane groups {2, 3} of slot j <-> lane groups {0, 1} of slot j + 2
    auto a = __builtin_amdgcn_permlane32_swap(lo[j], lo[j + 2], false, false);
    auto c = __builtin_amdgcn_permlane32_swap(hi[j], hi[j + 2], false, false);
    lo[j] = a[0];
    lo[j + 2] = a[1];
    hi[j] = c[0];
    hi[j + 2] = c[1];
  }
#pragma unroll
  for (int j = 0; j < 4; j += 2) {                           // odd lane groups of slot j <-> even lane groups of slot j + 1
    auto a = __builtin_amdgcn_permlane16_swap(lo[j], lo[j + 1], false, false);
    auto c = __builtin_amdgcn_permlane16_swap(hi[j], hi[j + 1], false, false);
    lo[j] = a[0];
    lo[j + 1] = a[1];
    hi[j] = c[0];
    hi[j + 1] = c[1];
  }
  e0 = __hiloint2double(hi[0], lo[0]);
  e1 = __hiloint2double(hi[1], lo[1]);
  e2 = __hiloint2double(hi[2], lo[2]);
  e3 = __hiloint2double(hi[3], lo[3]);
}
__device__ __forceinline__ bool rows_as_lines(const void *base, int64_t ld, int D, int DP) {
  return D == DP && DP >= 16 && (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
}
// xo[ks] = row[4 ks + lgrp] for the lane's frame (`row` = its first feature; zero when !live or beyond D).  ALL lanes of the
// wave must call it (the transpose exchanges registers across lanes); a frame that is not live passes any valid row.
template <int KS>
__device__ __forceinline__ void load_frame_row(const double *row, bool live, bool lines, int D, int lgrp, double (&xo)[KS]) {
  constexpr int NB = KS / 4;
  if (lines) {
    typedef double xd2 __attribute__((ext_vector_type(2)));
    xd2 v[NB > 0 ? NB : 1][2];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      v[b][0] = *reinterpret_cast<const xd2 *>(row + 16 * b + 4 * lgrp);
      v[b][1] = *reinterpret_cast<const xd2 *>(row + 16 * b + 4 * lgrp + 2);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      double e0 = v[b][0].x, e1 = v[b][0].y, e2 = v[b][1].x, e3 = v[b][1].y;
      transpose_lane_groups4(e0, e1, e2, e3);
      xo[4 * b] = live ? e0 : 0.0;
      xo[4 * b + 1] = live ? e1 : 0.0;
      xo[4 * b + 2] = live ? e2 : 0.0;
      xo[4 * b + 3] = live ? e3 : 0.0;
    }
#pragma unroll
    for (int ks = 4 * NB; ks < KS; ++ks) xo[ks] = live ? row[4 * ks + lgrp] : 0.0;
  } else {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = 4 * ks + lgrp;
      xo[ks] = (live && k < D) ? row[k] : 0.0;
    }
  }
}
// x[f][ks] = row[f][4 ks + lgrp] for the lane's frame of tile f (`row[f]` = its first feature; zero when !live[f] or beyond D), in
// two halves, so that ALL tiles' rows are in flight before the wave waits for the first (one memory round trip instead of one
// per tile) and the caller can issue more between the halves.  request_frame_rows only issues the loads, into the registers
// of x themselves: 32 contiguous bytes per block of the line path (LINES), single features of its tail and of the other
// path.  Every address is valid whatever `live` says: a frame that is not live passes any valid row, a feature beyond D reads
// feature 0 (only the last k-step can hold one: D > 4 (KS - 1)) -- a load under an exec branch is one the compiler does not
// batch with its neighbours.  finish_frame_rows does the transposes and the masking in place.  ALL lanes of the wave must
// call both (the transpose exchanges registers across lanes).  LINES is a template argument so that a caller branches ONCE
// around request, whatever it issues in between, and finish: with the branch inside the halves the compiler merges the two
// paths' tails and puts a wait between a tile's blocks and its tail.
template <int KS, int FT, bool LINES>
__device__ __forceinline__ void request_frame_rows(const double *const (&row)[FT], int D, int lgrp, double (&x)[FT][KS]) {
  constexpr int NB = KS / 4;
  if constexpr (LINES) {
    typedef double xd2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int f = 0; f < FT; ++f) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const xd2 v0 = *reinterpret_cast<const xd2 *>(row[f] + 16 * b + 4 * lgrp);
        const xd2 v1 = *reinterpret_cast<const xd2 *>(row[f] + 16 * b + 4 * lgrp + 2);
        x[f][4 * b] = v0.x;
        x[f][4 * b + 1] = v0.y;
        x[f][4 * b + 2] = v1.x;
        x[f][4 * b + 3] = v1.y;
      }
#pragma unroll
      for (int ks = 4 * NB; ks < KS; ++ks) x[f][ks] = row[f][4 * ks + lgrp];      // (LINES: D is the padded dimension)
    }
  } else {
    const int klast = (4 * (KS - 1) + lgrp < D) ? 4 * (KS - 1) + lgrp : 0;
#pragma unroll
    for (int f = 0; f < FT; ++f) {
#pragma unroll
      for (int ks = 0; ks < KS - 1; ++ks) x[f][ks] = row[f][4 * ks + lgrp];
      x[f][KS - 1] = row[f][klast];
    }
  }
}
template <int KS, int FT, bool LINES>
__device__ __forceinline__ void finish_frame_rows(const bool (&live)[FT], int D, int lgrp, double (&x)[FT][KS]) {
  constexpr int NB = KS / 4;
#pragma unroll
  for (int f = 0; f < FT; ++f) {
    if constexpr (LINES) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        double e0 = x[f][4 * b], e1 = x[f][4 * b + 1], e2 = x[f][4 * b + 2], e3 = x[f][4 * b + 3];
        transpose_lane_groups4(e0, e1, e2, e3);
        x[f][4 * b] = live[f] ? e0 : 0.0;
        x[f][4 * b + 1] = live[f] ? e1 : 0.0;
        x[f][4 * b + 2] = live[f] ? e2 : 0.0;
        x[f][4 * b + 3] = live[f] ? e3 : 0.0;
      }
#pragma unroll
      for (int ks = 4 * NB; ks < KS; ++ks) x[f][ks] = live[f] ? x[f][ks] : 0.0;
    } else {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) x[f][ks] = (live[f] && (ks < KS - 1 || 4 * ks + lgrp < D)) ? x[f][ks] : 0.0;
    }
  }
}
// both halves with `between()` issued after the requests (more loads, a DMA, a wait): one branch on `lines` around the three
template <int KS, int FT, class Between>
__device__ __forceinline__ void load_frame_rows(const double *const (&row)[FT], const bool (&live)[FT], bool lines, int D, int lgrp,
                                                double (&x)[FT][KS], Between &&between) {
  if (lines) {
    request_frame_rows<KS, FT, true>(row, D, lgrp, x);
    between();
    finish_frame_rows<KS, FT, true>(live, D, lgrp, x);
  } else {
    request_frame_rows<KS, FT, false>(row, D, lgrp, x);
    between();
    finish_frame_rows<KS, FT, false>(live, D, lgrp, x);
  }
  // (each value through an empty asm: the finished operands are then registers of their own.  Without it they stay tied to the
  // 128-bit load tuples, all of which are in flight at once here, and the two-tile screen kernel at D = 40, which has no register
  // to spare at three waves per SIMD, spills 46 of them)
#pragma unroll
  for (int f = 0; f < FT; ++f) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(x[f][ks]));
  }
}
// row[4 j + lgrp] = yo[j] for the lane's frame; ALL lanes of the wave must call it
template <int KS>
__device__ __forceinline__ void store_frame_row(double *row, bool live, bool lines, int D, int lgrp, const double (&yo)[KS]) {
  constexpr int NB = KS / 4;
  if (lines) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      double e0 = yo[4 * b], e1 = yo[4 * b + 1], e2 = yo[4 * b + 2], e3 = yo[4 * b + 3];
      transpose_lane_groups4(e0, e1, e2, e3);
      if (live) {
        typedef double yd2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<yd2 *>(row + 16 * b + 4 * lgrp) = yd2{e0, e1};
        *reinterpret_cast<yd2 *>(row + 16 * b + 4 * lgrp + 2) = yd2{e2, e3};
      }
    }
  }
  if (live) {
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int r = 4 * j + lgrp;
      if ((!lines || j >= 4 * NB) && r < D) row[r] = yo[j];
    }
  }
}

}  // namespace vcmi
