// gmmmap_layout.hpp -- what the host packers (gmmmap_prepare.cpp) and the kernels (gmmmap.hip, gmmmap_screen.hpp, gmmmap_group.hip) must agree
// on, written down once: the row tiling of [U_m ; A_m] and the issue order of its operand fragments, the lane rule of an
// FP64 MFMA A-operand fragment, the stage layouts of the screens and the operands of the frame grouping.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace vcmi {

// ------------------------------------------------------------------------------------------------
// the row tiling for a padded dimension DP (multiple of 4)
// ------------------------------------------------------------------------------------------------
// MFMA kernel data layout: the 2*DP rows [U_m ; A_m] are cut into 16-row tiles; U-only tiles skip the k-steps that are
// entirely above the diagonal.  uonly: only the whitening rows U_m (log-density / posterior / argmax path: the regression
// rows are not staged).  The kernels see it through Tiling<DP, UONLY> below, the packers with the model's DP at run time.
struct TilingRT {
  // KS: k-steps covering all of x; NT: 16-row tiles over [U rows ; A rows]; NU: tiles that contain at least one U row
  int DP = 0, KS = 0, NT = 0, NU = 0, NSTEPS = 0;
  // per-mixture block in doubles: [fragments NSTEPS*64 | cinit NT*16 | lc | pad], multiple of 32 doubles (BLK: whole double2
  // per thread for 256- and 512-thread groups)
  int CINIT_OFF = 0, LC_OFF = 0, BLK = 0;
  __host__ __device__ constexpr explicit TilingRT(int dp, bool uonly = false) : DP(dp) {
    KS = DP / 4;
    NT = uonly ? (DP + 15) / 16 : (2 * DP + 15) / 16;
    NU = (DP + 15) / 16;
    NSTEPS = 0;
    for (int t = 0; t < NT; ++t) NSTEPS += steps(t);
    CINIT_OFF = NSTEPS * 64;
    LC_OFF = CINIT_OFF + NT * 16;
    BLK = ((LC_OFF + 1 + 1023) / 1024) * 1024;
  }
  __host__ __device__ constexpr int steps(int t) const {  // k-steps tile t needs
    return (16 * t + 15 < DP) ? ((4 * (t + 1) < KS) ? 4 * (t + 1) : KS) : KS;
  }
  // position of fragment (k-step ks, U tile t) in the k-step-major order of the U tiles (the order the packer writes them in)
  __host__ __device__ constexpr int ufrag_pos(int ks, int t) const {
    int n = 0;
    for (int k = 0; k < ks; ++k)
      for (int u = 0; u < NU && u < NT; ++u)
        if (k < steps(u)) ++n;
    for (int u = 0; u < t; ++u)
      if (ks < steps(u)) ++n;
    return n;
  }
  // fragments before tile t in that order: every U fragment comes before the first A tile
  __host__ __device__ constexpr int tile_off(int t) const { return t >= NU ? ufrag_pos(KS, 0) : 0; }
  // MODE 3 (predict with early exit) stores the whitening tiles one after the other in REVERSE order (tile NU-1 first):
  // rtile_off(i) = first fragment of the i-th tile in that order
  __host__ __device__ constexpr int rtile_off(int i) const {
    int n = 0;
    for (int u = 0; u < i; ++u) n += steps(NU - 1 - u);
    return n;
  }
};

// the same description as compile-time constants of a kernel instantiation
template <int DP, bool UONLY = false>
struct Tiling {
  static constexpr TilingRT RT = TilingRT(DP, UONLY);      // (read in constant expressions only)
  static constexpr int KS = RT.KS, NT = RT.NT, NU = RT.NU, NSTEPS = RT.NSTEPS, CINIT_OFF = RT.CINIT_OFF, LC_OFF = RT.LC_OFF, BLK = RT.BLK;
  __host__ __device__ static constexpr int steps(int t) { return TilingRT(DP, UONLY).steps(t); }
  __host__ __device__ static constexpr int tile_off(int t) { return TilingRT(DP, UONLY).tile_off(t); }
  __host__ __device__ static constexpr int ufrag_pos(int ks, int t) { return TilingRT(DP, UONLY).ufrag_pos(ks, t); }
  __host__ __device__ static constexpr int rtile_off(int i) { return TilingRT(DP, UONLY).rtile_off(i); }
  __host__ __device__ static constexpr int nsteps() { return NSTEPS; }
};

// Issue order of a mixture's operand fragments: fn(tile, k-step) for fragment 0, 1, ... NSTEPS-1 of its block.
//   variant 0: [U ; A] (convert) -- phase U k-major over the U tiles, then phase A k-major over the A tiles
//   variant 1: U only (log-densities, predict; the on-device packer's table) -- phase U alone
//   variant 2: U only, tile by tile with the LAST tile first (predict with early exit, MODE 3)
// tl is TilingRT(DP, variant != 0); the U tiles are tiles 0 .. NU-1 (NU <= NT).
template <class Fn>
inline void for_each_fragment(const TilingRT &tl, int variant, Fn fn) {
  if (variant == 2) {
    for (int t = tl.NU - 1; t >= 0; --t)
      for (int ks = 0; ks < tl.steps(t); ++ks) fn(t, ks);
    return;
  }
  for (int phase = 0; phase < 2; ++phase) {
    const int t0 = phase == 0 ? 0 : tl.NU, t1 = phase == 0 ? tl.NU : tl.NT;
    for (int ks = 0; ks < tl.KS; ++ks)
      for (int t = t0; t < t1; ++t)
        if (ks < tl.steps(t)) fn(t, ks);
  }
}

// ------------------------------------------------------------------------------------------------
// the lane rule of a 16 x 4 FP64 MFMA A-operand fragment (v_mfma_f64_16x16x4_f64): lane l holds row l & 15 of the tile
// and column l >> 4 of the k-step
// ------------------------------------------------------------------------------------------------
constexpr int frag_row(int l) { return l & 15; }
constexpr int frag_col(int l) { return l >> 4; }
// dst[0 .. 63] = the fragment of k-step ks: f(row of the tile, k = 4 ks + column)
template <class Fn>
inline void fill_fragment(double *dst, int ks, Fn f) {
  for (int l = 0; l < 64; ++l) dst[l] = f(frag_row(l), 4 * ks + frag_col(l));
}

// ------------------------------------------------------------------------------------------------
// which padded dimensions have kernels
// ------------------------------------------------------------------------------------------------
// The instantiation lists, written once: X(DP) for every padded dimension of the bf16 screen (.._40), of the screen kernels of
// shape 3 (.._48) and of the tile kernel, predict's screen and the grouping keys (all of them).  The switches of gmmmap.hip and
// gmmmap_group.hip expand them; the predicates below answer for the same sets (checked at compile time).
#define VCMI_TILE_DIMS_40(X) X(16) X(20) X(24) X(28) X(32) X(36) X(40)
#define VCMI_TILE_DIMS_48(X) VCMI_TILE_DIMS_40(X) X(44) X(48)
#define VCMI_TILE_DIMS(X) VCMI_TILE_DIMS_48(X) X(52) X(56) X(60) X(64) X(68) X(72) X(76) X(80)
// the tile kernel (gmmmap_mfma_kernel): DP = 16, 20, ... 80
constexpr bool gmmmap_has_mfma(int DP) { return DP >= 16 && DP <= 80 && DP % 4 == 0; }
// shape 3 (gmmmap_screen.hpp): DP = 16..48, any M up to 1024 (the survivors' bitmap)
constexpr bool screen_has_kernel(int DP) { return DP >= 16 && DP <= 48 && DP % 4 == 0; }

// ------------------------------------------------------------------------------------------------
// stage layouts of the screens (gmmmap_screen.hpp)
// ------------------------------------------------------------------------------------------------
// ROWS PER MIXTURE (rpm, chosen per model by choose_screen_rows(), gmmmap_prepare.cpp: the fewest rows that still rule (almost) every wrong mixture out):
//   4: lane group j of a screening tile = mixture j's four strongest rows               ->  4 mixtures per tile
//   2: registers {0,1} of lane group j = mixture 2j's two strongest rows, {2,3} = mixture 2j+1's  ->  8 mixtures per tile
//   1: register r of lane group j = the strongest row of mixture 4j + r                  -> 16 mixtures per tile (KS MFMAs screen 16)
// screening tiles per stage (one barrier per stage: 16 / 32 / 64 mixtures at four): two beyond DP = 48, where a stage of four
// would no longer leave room for two workgroups per CU beside the 32 KB whitening block
__host__ __device__ constexpr int screen_quads(int DP) { return DP <= 48 ? 4 : 2; }

// stage layout in doubles: [QS x KS x 64 operand fragments | QS x 4 lane groups x 8 {cinit r = 0..3, lc of sub-mixture 0..3}], whole KB
__host__ __device__ constexpr int screen_frag_doubles(int DP) { return screen_quads(DP) * (DP / 4) * 64; }
__host__ __device__ constexpr int screen_stage_doubles(int DP) { return (screen_frag_doubles(DP) + screen_quads(DP) * 32 + 127) / 128 * 128; }
// which mixture (relative to the tile's first) and which of its screening rows (0 = the strongest) tile row i stands for
__host__ __device__ constexpr int screen_row_mixture(int i, int rpm) { return (4 / rpm) * (i & 3) + (i >> 2) / rpm; }
__host__ __device__ constexpr int screen_row_index(int i, int rpm) { return (i >> 2) % rpm; }
// stages that hold M mixtures at rpm rows each
constexpr int screen_stage_count(int DP, int M, int rpm) { return (M + (16 / rpm) * screen_quads(DP) - 1) / ((16 / rpm) * screen_quads(DP)); }

// ---- the screen on the BF16 matrix pipe (B16 = true; rpm = 4, DP <= 40) --------------------------------------------------
// The screen only has to produce a CERTIFIED lower bound of sum_i a_i^2, a_i = P_i x - c_i.  v_mfma_f32_16x16x32_bf16 runs
// at 16x the FP64 MFMA rate, so P and x are split into two bf16 pieces each (hi + lo: 16 of their 53 bits) and
//   a^ = Ph xh + Ph xl + Pl xh - c      (three K = 32 instructions over the first eight k-steps of the FP64 operand layout -- lane
//                                        group g, slot j <-> feature 4 j + g, exactly what the lane's xb[.][j] holds -- and one
//                                        more whose slots carry the three terms of k-steps 8, 9), accumulated in FP32.
// |a^ - a| <= (dropped Pl xl and the two split residuals: 3 x 2^-16; FP32 accumulation of <= 130 exact products: 2^-15)
//             x sum_k |P_ik||x_k|  +  2^-24 |c_i|   <=   eps_i := 2^-12 (|P_i| |x| + |c_i|)       (Cauchy-Schwarz; ~2 x the sum above),
// so  a_i^2 >= max(|a^_i| - eps_i, 0)^2  and  lc - sum_i max(|a^_i| - eps_i, 0)^2 / 2  is still an upper bound of the mixture's
// log-density: a mixture it rules out is ruled out.  eps is ~0.3 where the test needs |a| of 10 and more: what the screen
// decides hardly changes, its matrix work drops from 10 FP64 MFMAs (640 cycles) to 4 BF16 ones (64 cycles) per tile.
// The FP32 result layout gives lane group j rows 4 j .. 4 j + 3: tile row i <-> mixture i >> 2, screening row i & 3.
// The margins and the sum of squares are formed in FP32 (the FP64 vector pipe is the one the conversion itself needs): the
// constants are rounded UP on the host (and carry a factor 1 + 2^-20 for the FP32 roundings of eps), the sum is taken down by
// 1 - 2^-20 before it is used.
// Stage layout in doubles: per tile [Ph main | Pl main | tail] as 3 x 1 KB of bf16x8 per lane, then per tile and lane group
// 8 doubles {c_0..3 (4 floats), 2^-12 |P_0..3| (4 floats), 2^-12 |c_0..3| (4 floats), lc (double), pad}.
__host__ __device__ constexpr int screen16_tile_doubles() { return 3 * 128; }
__host__ __device__ constexpr int screen16_stage_doubles(int DP) { return screen_quads(DP) * (screen16_tile_doubles() + 32); }
__host__ __device__ constexpr bool screen16_has(int DP) { return DP >= 16 && DP <= 40 && DP % 4 == 0; }

// the three predicates are true exactly on their lists
#define VCMI_DIM_IS(DPV) || DP == DPV
constexpr bool tile_dims_agree() {
  for (int DP = -4; DP <= 256; ++DP)
    if (gmmmap_has_mfma(DP) != (false VCMI_TILE_DIMS(VCMI_DIM_IS)) || screen_has_kernel(DP) != (false VCMI_TILE_DIMS_48(VCMI_DIM_IS)) ||
        screen16_has(DP) != (false VCMI_TILE_DIMS_40(VCMI_DIM_IS)))
      return false;
  return true;
}
#undef VCMI_DIM_IS
static_assert(tile_dims_agree(), "gmmmap_has_mfma / screen_has_kernel / screen16_has and the VCMI_TILE_DIMS lists disagree");

// ---- the second look of the bf16 screen: sixteen rows of ONE mixture per tile (packedQ2, pack_screen2_bf16) ----------------
// A mixture that its four strongest rows do not rule out is looked at once more with the min(16, D) strongest rows of the same
// eigen-expansion before it becomes a survivor: the same four instructions against the same B operands, the same margins per
// row, so  lc - sum_{i < 16} max(|a^_i| - eps_i, 0)^2 / 2  is an upper bound of the log-density as well, and never above the
// four-row one (rows 0..3 are the four-row screen's, the other terms are >= 0).  One tile per mixture in the layout of one
// tile of a bf16 stage: [Ph main | Pl main | tail] as 3 x 1 KB of bf16x8 per lane, tile row r = the mixture's row r (so lane
// group j of the FP32 result holds rows 4 j .. 4 j + 3; rows from D on are zero), then ONE constant line of 32 doubles: per
// lane group j 8 doubles {c_4j..4j+3 (4 floats), 2^-12 |P_4j..4j+3| (4 floats), 2^-12 |c_4j..4j+3| (4 floats), lc (double), pad}.
// The kernel reads a tile straight from global memory (the image is 3.3 KB per mixture and stays in L2).
__host__ __device__ constexpr int screen2_rows() { return 16; }
__host__ __device__ constexpr int screen2_const_off() { return screen16_tile_doubles(); }       // doubles from the tile's start
__host__ __device__ constexpr int screen2_tile_doubles() { return screen16_tile_doubles() + 32; }
constexpr size_t screen2_doubles(int M) { return (size_t)M * screen2_tile_doubles(); }

// ------------------------------------------------------------------------------------------------
// operands of fvconvert's frame grouping (gmmmap_group_key_kernel / gmmmap_group_key16_kernel, gmmmap_group.hip)
// ------------------------------------------------------------------------------------------------
constexpr int kGroupKeyDims = 24;     // dimensions the nearest-mean key is taken over (a multiple of 4)
constexpr int kKey16TileBytes = 2 * 1024 + 64;   // per 16 mixtures: 64 x 16 bytes of hi, 64 x 16 bytes of lo, 4 x 4 floats of |mu|^2
// gfrag[mt][ks][lane]: one fragment per k-step the key looks at and one more that carries |mu|^2
constexpr size_t group_key_doubles(int DP, int M) {
  return (size_t)((M + 15) / 16) * ((DP / 4 < kGroupKeyDims / 4 ? DP / 4 : kGroupKeyDims / 4) + 1) * 64;
}
constexpr size_t group_key16_doubles(int M) { return (size_t)((M + 15) / 16) * (kKey16TileBytes / 8); }

}  // namespace vcmi
