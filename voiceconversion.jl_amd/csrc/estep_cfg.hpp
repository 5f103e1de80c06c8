// estep_cfg.hpp -- the compile-time configuration of the diagonal E-step: the tile and LDS layouts of its four MFMA kernels, the
// sizes its launches are cut by, the ladder of instantiated joint dimensions and the shapes the MFMA kernels serve.  Pure
// constexpr, no HIP: the kernel headers (estep_mfma.hpp, estep_wave.hpp, estep_small.hpp, estep_hard.hpp, estep_path.hpp) and
// the host-only launch plan (estep_plan.cpp) read the same numbers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace vcmi {

// doubles of the packed statistics [S0 (M) | S1 (Dj,M) | S2 (Dj,M) | loglik]: what vcmi_estep_stats_len returns
constexpr int64_t estep_stats_len(int Dj, int M) { return (int64_t)M * (1 + 2 * Dj) + 1; }

// ---- generic kernels (estep_generic.hpp) ----
constexpr int kChunk = 1 << 16;   // frames per workspace chunk
constexpr int kSeg = 512;         // frames per deterministic accumulation segment

// ---- estep_mfma_kernel (estep_mfma.hpp) ----
// Dj a multiple of 16 (at Dj = 80: K = 160 = [x^2 | x], 40 k-steps; 10 statistic column tiles [x | x^2]).
// Up to Dj = 80 one kernel; above as two (SPLIT below).
template <int DJ>
struct EstepCfg {
  static constexpr int KS = 2 * DJ / 4;          // k-steps of the log-density contraction
  static constexpr int NDT = 2 * DJ / 16;        // 16-wide column tiles of the statistics [x | x^2]
  // A workgroup keeps its slice of W (M x 2 DJ) and of the statistics (M x 2 DJ) in registers: 2 x 164 KB at DJ = 80,
  // M = 128.  Beyond that the two do not fit the 512 KB register file of a CU together, and the E-step runs as TWO
  // kernels -- responsibilities (W in registers), then statistics (accumulators in registers) -- with gamma (N x 128)
  // through HBM in between: 2 x 1 KB per frame of extra traffic against 5 KB of x^2 / x operands per frame.
  static constexpr bool SPLIT = DJ > 80;
  static constexpr int FB = SPLIT ? 32 : 64;     // frames per block
  // LDS row stride of x (doubles): a multiple of 16 bytes (LDS-DMA rows) and == 18 mod 32, i.e. 36 mod 64 in dwords ->
  // step A's 16-row column reads hit distinct banks
  static constexpr int RSX = (DJ + 2 + 13) / 32 * 32 + 18;
  static constexpr int XBUF = (FB * RSX * 8 + 1023) / 1024 * 128;   // doubles per x buffer: whole 1 KB wave-instructions of the DMA
  static constexpr int MMAX = 128;               // 8 waves x 16 mixtures
  static constexpr int RSG = MMAX + 16;          // LDS row stride of gamma; == 16 mod 32 -> f-groups land 32 banks apart
  // two x buffers (block k+1 streams in by LDS-DMA while block k is processed) + l/gamma; the log-likelihood scratch of
  // the epilogue aliases the l/gamma area
  // + the 2^(j/64) table of vc_exp_tab (64 doubles) + step B's frame order: winning tile per frame (FB ints) and one
  // permutation per wave (8 x FB ints)
  // + the refinement thresholds of the 128 mixture slots (see estep_prep_kernel)
  static constexpr size_t LDS_BYTES = ((size_t)2 * XBUF + (size_t)FB * RSG + 64 + MMAX) * sizeof(double) + (size_t)9 * FB * sizeof(int);
  static_assert(RSX >= DJ + 2 && RSX % 2 == 0, "row stride");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};
constexpr int64_t kSplitChunk = (int64_t)1 << 20;      // frames per chunk of the two-kernel (SPLIT) form: bounds gamma in HBM
constexpr int64_t kPadChunk = (int64_t)1 << 20;        // frames per chunk of an odd joint dimension: bounds the padded copy
constexpr int64_t kGroupsChunk = (int64_t)1 << 18;     // frames per chunk of more than 128 mixtures: bounds gamma of every group
constexpr int kCombineGrid = 1024;                     // workgroups of estep_group_combine_kernel (= its log-likelihood partials)

// ---- estep_wave_kernel (estep_wave.hpp) ----
template <int DJ>
struct EstepWaveCfg {
  static constexpr int KS = 2 * DJ / 4, NDT = 2 * DJ / 16;
  static constexpr int FB = 32;                                  // frames per block
  static constexpr int RSX = (DJ + 2 + 13) / 32 * 32 + 18;       // as EstepCfg: 16-byte rows, conflict-free column reads
  static constexpr int XBUF = FB * RSX;                          // doubles per x buffer (the last 1 KB wave-instruction of the DMA is masked)
  static constexpr int NXB = 4;
  // a private plane holds value (frame f, mixture c of the wave's 16) at (c & 7) * PROW + 2 f + (c >> 3): the softmax lanes
  // (lane = 2 f + half, value i = c & 7) read and write stride-1 across the wave, step A's stores (rows of 8 dwords, 8 dwords
  // apart) are conflict-free too; the 4 spare doubles of each row hold 1 / S of the block's frames (step B)
  static constexpr int PROW = 2 * FB + 4;
  static constexpr int PLANE = 8 * PROW;                         // doubles per private plane (l, then e in place); two per wave
  static constexpr int XSET = 8 * FB;                            // doubles per table set: [wave][frame]
  // doubles: [x NXB][planes 8 x 2][maxima 2 sets][sums 2 sets][etab 64]; bytes: [counts 2 x 8 x FB][frame order 8 x FB]
  static constexpr size_t LDS_DOUBLES = (size_t)NXB * XBUF + 16 * PLANE + 4 * XSET + 64;
  static constexpr size_t LDS_BYTES = LDS_DOUBLES * 8 + (size_t)2 * 8 * FB + 8 * FB;
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

// ---- estep_small_kernel (estep_small.hpp) ----
template <int DJ, int MT>
struct EstepSmallCfg {
  static_assert(MT == 1 || MT == 2, "one or two mixture tiles");
  static constexpr int KS = 2 * DJ / 4, NDT = 2 * DJ / 16;
  static constexpr int NW = 2 * MT;                              // waves per workgroup
  // frames per block.  MT = 2: two frame tiles of 16, a wave = (mixture tile, frame tile) in step A.  MT = 1: ONE frame tile,
  // and the two waves split the contraction of step A by k-steps (partial sums in two planes of LDS, added by the softmax) --
  // half the LDS per workgroup, so that four of them fit a CU and every SIMD has its two waves (with 32-frame blocks a CU
  // held two workgroups of two waves: one wave per SIMD, 0.55 ms per 1.25e6 frames at M = 16)
  static constexpr int FB = MT == 1 ? 16 : 32;
  static constexpr bool SPLITK = MT == 1;
  static constexpr int PLANES = SPLITK ? 2 : 1;
  static constexpr int RSX = (DJ + 2 + 13) / 32 * 32 + 18;       // as EstepCfg: 16-byte rows, conflict-free column reads
  static constexpr int NCHUNK = (FB * RSX * 8 + 1023) / 1024;    // 1 KB wave-instructions of the LDS-DMA per x image
  // doubles between two x images.  MT = 1: exactly the image -- the last wave-instruction of an image is cut off behind it
  // (kLastLanes) -- because there every byte counts: four workgroups per CU have 40 KB each
  static constexpr int XBUF = SPLITK ? FB * RSX : NCHUNK * 128;
  static constexpr int kLastLanes = SPLITK ? (FB * RSX * 8 - 1024 * (NCHUNK - 1)) / 16 : 64;
  static constexpr int NV = 16 * MT * FB / (64 * NW);            // softmax values per lane: 4 (MT = 2) / 2 (MT = 1)
  static constexpr int LPF = 16 * MT / NV;                       // softmax lanes per frame
  static_assert(LPF == 8 && 64 / LPF * NW == FB, "one softmax pass per wave and block");
  // LDS row stride of l / gamma (doubles): the softmax's half-wave (four frames x eight consecutive doubles) lands on 64
  // distinct banks -- MT = 2: rows 80 dwords apart -> 0, 16, 32, 48 mod 64; MT = 1: 48 dwords -> 0, 48, 32, 16
  static constexpr int RSG = MT == 2 ? 40 : 24;
  static constexpr int WG_PER_CU = MT == 2 ? 2 : 4;
  // [x 3][l / gamma PLANES x FB x RSG][etab 64][thresholds 16 MT] doubles + [DMA source offsets: NCHUNK x 64 lanes] shorts
  static constexpr size_t LDS_BYTES = ((size_t)3 * XBUF + (size_t)PLANES * FB * RSG + 64 + 16 * MT) * sizeof(double) + (size_t)NCHUNK * 64 * sizeof(unsigned short);
  static_assert(FB * 80 * 8 < 65536 && (XBUF * 8) % 16 == 0, "offsets fit 16 bits; images are 16-byte aligned");
  static_assert(LDS_BYTES * WG_PER_CU <= 160 * 1024, "LDS");
};

// ---- the hard-assignment path (estep_hard.hpp, estep_path.hpp) ----
constexpr int kHardPiece = 256;        // hard frames per workgroup of the statistics kernel
constexpr int kHardMaxM = 128;         // mixtures (the one-kernel path's limit; more go through the groups of estep_groups_launch)
constexpr int kHardKeyThreads = 512;   // one workgroup per CU (the operands of all mixtures fill half its LDS): eight waves of two frame tiles each (256 registers: sixteen waves of two tiles spill at Dj = 80)
constexpr int64_t kHardMinFrames = 65536;      // fewer frames: the one-kernel path without a look at the data
constexpr int kHardChunk = 1024;       // frames per chunk of the keys' histograms and the sort: kGroupChunk (grouping.hpp)
constexpr int kHardSamplePasses = kHardChunk / (32 * (kHardKeyThreads / 64));      // run units per sampled chunk (one pass each)
// W in bf16 for the key kernel: per mixture tile mt (16 mixtures) and instruction i (x dimensions 16 i .. 16 i + 15):
// [hi 64 x 16 B | lo 64 x 16 B]; slot j of lane group g <-> j < 4: -1/(2 var) of dimension 16 i + 4 g + j (multiplies x^2),
// j >= 4: mu / var of dimension 16 i + 4 g + (j - 4) (multiplies x).  Then per tile 48 floats: c (16), 2^-12 |W_m| (16, rounded
// up), 2^-12 |c_m| (16, rounded up); a mixture without weight or beyond M: c = -1e30, margins 0 (its l^ is certified hopeless).
template <int DJ>
struct EstepHardCfg {
  static constexpr int NI = (DJ + 15) / 16;                  // K = 32 instructions per term
  static constexpr int TILE_BYTES = NI * 2048 + 192;         // operands of one mixture tile
  static constexpr size_t lds_bytes(int mt) { return (size_t)mt * TILE_BYTES; }
};
// ctl (int64, device): [0] 1: the hard-assignment path runs / 0: every frame through estep_mfma_kernel; [1] frames of the
// "everything soft" launch (N or 0); [2] soft frames found by the hard-assignment path (estep_hard_gather_kernel)
enum { kCtlHard = 0, kCtlAllSoft = 1, kCtlNSoft = 2, kCtlLen = 4 };

// ---- which joint dimensions and shapes the MFMA kernels serve ----
// The smallest instantiation DJ that holds Dj: 32, 48, 64, 80 (one kernel), then the two-kernel form -- 112 for the dimensions
// between (Dj = 82 ... 112 ran in the 160-wide one: 1.5 x the work)
constexpr int estep_mfma_dj(int Dj) { return Dj <= 32 ? 32 : Dj <= 48 ? 48 : Dj <= 64 ? 64 : Dj <= 80 ? 80 : Dj <= 112 ? 112 : 160; }
// f(std::integral_constant<int, DJ>) for DJ = estep_mfma_dj(Dj)
template <class F>
int with_mfma_dj(int Dj, const F &f) {
  switch (estep_mfma_dj(Dj)) {
    case 32: return f(std::integral_constant<int, 32>{});
    case 48: return f(std::integral_constant<int, 48>{});
    case 64: return f(std::integral_constant<int, 64>{});
    case 80: return f(std::integral_constant<int, 80>{});
    case 112: return f(std::integral_constant<int, 112>{});
    default: return f(std::integral_constant<int, 160>{});
  }
}
// The joint dimensions the MFMA kernels serve: even (the rows of X are 16-byte aligned for the LDS-DMA), up to 160
// (generic: the test hook kDbgEstepGeneric, which the caller reads) ...
constexpr bool mfma_dims(int Dj, bool generic) { return Dj % 2 == 0 && Dj <= 160 && !generic; }
// ... and the shapes estep_mfma_launch serves among them: at most 128 mixtures (more run as groups of 128)
constexpr bool estep_mfma_shape(int Dj, int M, bool generic) { return M <= EstepCfg<80>::MMAX && mfma_dims(Dj, generic); }

}  // namespace vcmi
