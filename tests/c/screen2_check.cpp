// screen2_check.cpp -- the second look of the bf16 screen (csrc/gmmmap_screen.hpp, step 2) replayed on the CPU from the image
// that pack_screen2_bf16() writes: sixteen rows of one mixture per tile (csrc/gmmmap_layout.hpp: screen2_*).  Deterministic SPD
// models go through factor_model(); for a few hundred points -- near the means, and shifted by +300, -2000 and +50 in every
// feature -- and EVERY mixture the look's arithmetic is redone as the kernel does it: bf16 hi / lo operands read back from the
// image, the three-term product Ph xh + Ph xl + Pl xh accumulated in FP32, the margins 2^-12 (|P_i| |x| + |c_i|) from the image's
// constant line, the sum of squares in FP32 per lane group.  Checked: the image has the length the layout header gives; the
// certified bound is >= the exact log-density (hm.U, hm.cz, hm.lc in FP64) -- a mixture the look rules out IS out; and it is
// <= the four-row bound replayed the same way from pack_screen_bf16()'s image -- the look never keeps what the first one dropped.
// Built by tests/test_screen2_host.py with -fsanitize=address,undefined: a packer that writes past its image is a finding too.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../voiceconversion.jl_amd/csrc/bf16_split.hpp"
#include "../../voiceconversion.jl_amd/csrc/gmmmap_prepare.hpp"

using namespace vcmi;

static int bad = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (++bad <= 20) printf("screen2_check: D=%d M=%d: %s\n", D, M, #cond); \
    }                                                               \
  } while (0)

struct Lcg {      // deterministic uniform deviates in (-1, 1)
  unsigned long long s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((s >> 11) & ((1ull << 53) - 1)) * (2.0 / 9007199254740992.0) - 1.0;
  }
};

static float bf(unsigned short h) {
  unsigned u = (unsigned)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// One tile of bf16 operands ([Ph | Pl | tail], 3 x 1 KB, lane l = 16 (feature & 3) + tile row) against one frame: the FP32
// results of the tile's sixteen rows, a[r] = -c[r] + sum_k (Ph xh + Ph xl + Pl xh), the products in the order of the kernel's
// four instructions.  cst(r) -> {c, 2^-12 |P|, 2^-12 |c|} of tile row r; t2[r] = max(|a_r| - eps_r, 0).
template <class Cst>
static void tile_rows(const unsigned short *fr, int KS, const unsigned short *xh, const unsigned short *xl, float nxf, Cst cst, float *t2) {
  const int NMAIN = KS < 8 ? KS : 8;
  for (int r = 0; r < 16; ++r) {
    float c, np, nc;
    cst(r, c, np, nc);
    float a = -c;
    for (int pass = 0; pass < 3; ++pass)            // Ph xh, Ph xl, Pl xh over k-steps 0..7
      for (int g = 0; g < 4; ++g)
        for (int j = 0; j < NMAIN; ++j) {
          const int l = 16 * g + r, k = 4 * j + g;
          const float p = bf(fr[(pass == 2 ? 512 : 0) + (size_t)l * 8 + j]), x = bf(pass == 1 ? xl[k] : xh[k]);
          a += p * x;                                // (a product of two bf16 numbers is exact in FP32)
        }
    for (int g = 0; g < 4; ++g) {                    // tail slots {Ph8, Ph9, Ph8, Ph9, Pl8, Pl9, 0, 0} against {xh8, xh9, xl8, xl9, xh8, xh9, 0, 0}
      const int l = 16 * g + r;
      const unsigned short *tp = fr + 1024 + (size_t)l * 8;
      const unsigned short x8h = KS > 8 ? xh[32 + g] : 0, x9h = KS > 9 ? xh[36 + g] : 0, x8l = KS > 8 ? xl[32 + g] : 0, x9l = KS > 9 ? xl[36 + g] : 0;
      const unsigned short xs[8] = {x8h, x9h, x8l, x9l, x8h, x9h, 0, 0};
      for (int j = 0; j < 8; ++j) a += bf(tp[j]) * bf(xs[j]);
    }
    t2[r] = fmaxf(fabsf(a) - fmaf(np, nxf, nc), 0.0f);
  }
}

static void run(int D, int M) {
  const int Dj = 2 * D, DP = (D + 3) / 4 * 4, KS = DP / 4;
  Lcg rng{(unsigned long long)(7000003 * D + 131 * M)};
  std::vector<double> w(M), mu((size_t)Dj * M), sigma((size_t)Dj * Dj * M), B((size_t)Dj * Dj);
  double tot = 0.0;
  for (int m = 0; m < M; ++m) tot += (w[m] = (m == 1 ? 0.0 : 1.5 + rng.next()));      // one zero weight: lc = -inf
  for (int m = 0; m < M; ++m) w[m] /= tot;
  for (double &v : mu) v = 3.0 * rng.next();
  for (int m = 0; m < M; ++m) {      // B B' / Dj + a positive diagonal whose entries spread over three decades, column-major
    for (double &v : B) v = rng.next();
    double *S = &sigma[(size_t)Dj * Dj * m];
    for (int r = 0; r < Dj; ++r)
      for (int c = 0; c <= r; ++c) {
        double acc = 0.0;
        for (int k = 0; k < Dj; ++k) acc += B[(size_t)r * Dj + k] * B[(size_t)c * Dj + k];
        S[r + (size_t)Dj * c] = S[c + (size_t)Dj * r] = 0.05 * acc / Dj + (r == c ? std::pow(10.0, -3.0 * ((r * 7 + m) % 11) / 10.0) : 0.0);
      }
  }
  vcmi_gmmmap g;      // host copies only
  HostModel hm;
  CHECK(factor_model(&g, hm, w.data(), mu.data(), sigma.data(), Dj, M, 0, false) == VCMI_OK);
  CHECK(hm.P2.size() == (size_t)M * screen2_rows() * DP && hm.cP2.size() == (size_t)M * screen2_rows());
  if (bad) return;
  for (int m = 0; m < M; ++m)      // rows 0..3 are the four-row screen's; rows from D on are zero
    for (int r = 0; r < 4; ++r) {
      CHECK(memcmp(&hm.P2[((size_t)m * 16 + r) * DP], &hm.P[((size_t)m * 4 + r) * DP], DP * sizeof(double)) == 0);
      CHECK(hm.cP2[(size_t)m * 16 + r] == hm.cP[(size_t)m * 4 + r]);
    }
  const std::vector<double> p2 = pack_screen2_bf16(hm), p16 = pack_screen_bf16(hm);
  CHECK(p2.size() == screen2_doubles(M) && p2.size() == (size_t)M * screen2_tile_doubles());
  CHECK(p16.size() == (size_t)screen_stage_count(DP, M, 4) * screen16_stage_doubles(DP));
  if (bad) return;

  const int NP = 256, NQ = screen_quads(DP), STG16 = screen16_stage_doubles(DP);
  const double shifts[4] = {0.0, 300.0, -2000.0, 50.0};
  const double half = 0.5 * (1.0 - 0x1p-20);
  const size_t pp = (size_t)DP * DP;
  std::vector<double> x(DP);
  std::vector<unsigned short> xh(40), xl(40);
  int ruled_out16 = 0, ruled_out4 = 0;
  for (int i = 0; i < NP; ++i) {
    const int src = i % M;
    std::fill(x.begin(), x.end(), 0.0);
    double q = 0.0;
    for (int d = 0; d < D; ++d) {
      x[d] = g.h_mux[(size_t)D * src + d] + 0.05 * rng.next() + shifts[(i / M + i) % 4];
      q = std::fma(x[d], x[d], q);
    }
    std::fill(xh.begin(), xh.end(), 0);
    std::fill(xl.begin(), xl.end(), 0);
    for (int k = 0; k < DP; ++k) split_bf16(x[k], xh[k], xl[k]);
    const float nxf = (float)(std::sqrt(q) * (1.0 + 0x1p-20));
    double best = -INFINITY;
    std::vector<double> exact(M), b16(M), b4(M);
    for (int m = 0; m < M; ++m) {
      // the exact log-density
      double zz = 0.0;
      for (int r = 0; r < D; ++r) {
        double z = -hm.cz[(size_t)DP * m + r];
        for (int c = 0; c <= r; ++c) z += hm.U[pp * m + (size_t)r * DP + c] * x[c];
        zz += z * z;
      }
      exact[m] = hm.lc[m] - 0.5 * zz;
      best = std::fmax(best, exact[m]);
      float t2[16];
      // the second look: tile m of packedQ2, lane group j <-> rows 4 j .. 4 j + 3
      const double *tile = &p2[(size_t)m * screen2_tile_doubles()], *cl = tile + screen2_const_off();
      tile_rows(reinterpret_cast<const unsigned short *>(tile), KS, xh.data(), xl.data(), nxf,
                [&](int r, float &c, float &np, float &nc) {
                  const float *cf = reinterpret_cast<const float *>(cl + (r >> 2) * 8);
                  c = cf[r & 3];
                  np = cf[4 + (r & 3)];
                  nc = cf[8 + (r & 3)];
                },
                t2);
      float lb[4];
      for (int j = 0; j < 4; ++j) {
        lb[j] = 0.0f;
        for (int r = 0; r < 4; ++r) lb[j] = fmaf(t2[4 * j + r], t2[4 * j + r], lb[j]);
        double lcj;
        memcpy(&lcj, cl + j * 8 + 6, 8);
        CHECK(lcj == hm.lc[m] || (std::isinf(lcj) && std::isinf(hm.lc[m])));
      }
      b16[m] = std::fma(-half, ((double)lb[0] + (double)lb[1]) + ((double)lb[2] + (double)lb[3]), hm.lc[m]);
      // the four-row screen: tile (m / 4) of packedQ16, lane group m & 3 <-> the mixture's four rows
      const int st = m / (4 * NQ), qd = (m / 4) % NQ, j4 = m & 3;
      const double *tile4 = &p16[(size_t)st * STG16 + (size_t)qd * screen16_tile_doubles()];
      const double *cl4 = &p16[(size_t)st * STG16 + (size_t)NQ * screen16_tile_doubles() + (size_t)qd * 32];
      tile_rows(reinterpret_cast<const unsigned short *>(tile4), KS, xh.data(), xl.data(), nxf,
                [&](int r, float &c, float &np, float &nc) {
                  const float *cf = reinterpret_cast<const float *>(cl4 + (r >> 2) * 8);
                  c = cf[r & 3];
                  np = cf[4 + (r & 3)];
                  nc = cf[8 + (r & 3)];
                },
                t2);
      float l4 = 0.0f;
      for (int r = 0; r < 4; ++r) l4 = fmaf(t2[4 * j4 + r], t2[4 * j4 + r], l4);
      b4[m] = std::fma(-half, (double)l4, cl4[j4 * 8 + 6]);
      CHECK(b16[m] >= exact[m]);            // an upper bound of the log-density
      CHECK(b16[m] <= b4[m]);               // ... and never above the four-row one
    }
    for (int m = 0; m < M; ++m) {
      ruled_out16 += (b16[m] <= best - 46.0);
      ruled_out4 += (b4[m] <= best - 46.0);
    }
  }
  CHECK(ruled_out16 >= ruled_out4);
  printf("screen2_check: D=%d M=%d: of %d (point, mixture) pairs the four rows rule out %d, the sixteen %d\n", D, M, NP * M, ruled_out4, ruled_out16);
}

// beyond the bf16 screen's dimensions there is no second look: no sixteen-row image is kept on the host
static void run_without(int D, int M) {
  const int Dj = 2 * D;
  Lcg rng{(unsigned long long)(9000011 * D + M)};
  std::vector<double> w(M, 1.0 / M), mu((size_t)Dj * M), sigma((size_t)Dj * Dj * M, 0.0);
  for (double &v : mu) v = rng.next();
  for (int m = 0; m < M; ++m)
    for (int r = 0; r < Dj; ++r) sigma[(size_t)Dj * Dj * m + r + (size_t)Dj * r] = 0.5 + 0.1 * (r % 5);
  vcmi_gmmmap g;
  HostModel hm;
  CHECK(factor_model(&g, hm, w.data(), mu.data(), sigma.data(), Dj, M, 0, false) == VCMI_OK);
  CHECK(!screen16_has(hm.DP) && hm.P.size() == (size_t)M * 4 * hm.DP && hm.P2.empty() && hm.cP2.empty());
}

int main() {
  for (int D : {16, 38, 40})
    for (int M : {3, 64}) run(D, M);
  run_without(44, 3);
  run_without(52, 3);
  printf("screen2_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
