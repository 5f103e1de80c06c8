// prepare_check.cpp -- sanitizer driver for the host-side model preparation (csrc/gmmmap_prepare.cpp): deterministic SPD
// models go through the steps gmmmap_prepare() runs -- factor, profile, choose, then every packer -- on the CPU, without a
// device.  Built by tests/test_sanitizers.py with -fsanitize=address,undefined: a packer that writes past its image, or reads
// past a host image, is a finding.  Checked here: every image has exactly the length gmmmap_layout.hpp gives for it, the issue
// order visits NSTEPS fragments, and pack_screen(4) is predict's screen as this file spells it out.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../voiceconversion.jl_amd/csrc/gmmmap_prepare.hpp"

using namespace vcmi;

static int bad = 0;
#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) {                                                                    \
      ++bad;                                                                          \
      printf("prepare_check: D=%d M=%d px_only=%d: %s\n", D, M, (int)px_only, #cond); \
    }                                                                                 \
  } while (0)

// the compile-time view of the tiling is the run-time one
static_assert(Tiling<40>::NSTEPS == TilingRT(40).NSTEPS && Tiling<40>::BLK == TilingRT(40).BLK && Tiling<40, true>::NT == TilingRT(40, true).NT &&
                  Tiling<28, true>::rtile_off(1) == TilingRT(28, true).rtile_off(1) && Tiling<80>::ufrag_pos(3, 2) == TilingRT(80).ufrag_pos(3, 2),
              "Tiling<> takes its values from TilingRT");

struct Lcg {      // deterministic uniform deviates in (-1, 1)
  unsigned long long s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((s >> 11) & ((1ull << 53) - 1)) * (2.0 / 9007199254740992.0) - 1.0;
  }
};

// predict's screen (gmmmap_screen_argmax_kernel), spelled out: four rows per mixture; tile row i is screening row i >> 2 of
// mixture i & 3; the fragment of k-step ks holds (row i, column 4 ks + c) at 16 c + i
static std::vector<double> predict_screen(const HostModel &hm) {
  const int DP = hm.DP, M = hm.M, KS = DP / 4, NQ = screen_quads(DP), STG = screen_stage_doubles(DP);
  const int nst = (M + 4 * NQ - 1) / (4 * NQ);
  std::vector<double> pq((size_t)nst * STG, 0.0);
  for (int st = 0; st < nst; ++st)
    for (int q = 0; q < NQ; ++q) {
      const int m0 = (NQ * st + q) * 4;
      double *fr = &pq[(size_t)st * STG + (size_t)q * KS * 64], *cl = &pq[(size_t)st * STG + screen_frag_doubles(DP) + (size_t)q * 32];
      for (int ks = 0; ks < KS; ++ks)
        for (int c = 0; c < 4; ++c)
          for (int i = 0; i < 16; ++i) {
            const int m = m0 + (i & 3), row = i >> 2, k = 4 * ks + c;
            fr[(size_t)ks * 64 + 16 * c + i] = (m < M && k < DP) ? hm.P[((size_t)m * 4 + row) * DP + k] : 0.0;
          }
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + j;
        for (int r = 0; r < 4; ++r) cl[j * 8 + r] = (m < M) ? -hm.cP[(size_t)m * 4 + r] : 0.0;
        for (int u = 0; u < 4; ++u) cl[j * 8 + 4 + u] = (u == 0 && m < M) ? hm.lc[m] : -std::numeric_limits<double>::infinity();
      }
    }
  return pq;
}

static void run(int D, int M, bool px_only) {
  const int Dj = px_only ? D : 2 * D, DP = (D + 3) / 4 * 4;
  Lcg rng{(unsigned long long)(1000003 * D + 101 * M + (px_only ? 7 : 0))};
  std::vector<double> w(M), mu((size_t)Dj * M), sigma((size_t)Dj * Dj * M), B((size_t)Dj * Dj);
  double tot = 0.0;
  for (int m = 0; m < M; ++m) tot += (w[m] = 1.5 + rng.next());
  for (int m = 0; m < M; ++m) w[m] /= tot;
  for (double &v : mu) v = 3.0 * rng.next();
  for (int m = 0; m < M; ++m) {      // B B' / Dj + a positive diagonal, column-major (symmetric)
    for (double &v : B) v = rng.next();
    double *S = &sigma[(size_t)Dj * Dj * m];
    for (int r = 0; r < Dj; ++r)
      for (int c = 0; c <= r; ++c) {
        double acc = 0.0;
        for (int k = 0; k < Dj; ++k) acc += B[(size_t)r * Dj + k] * B[(size_t)c * Dj + k];
        S[r + (size_t)Dj * c] = S[c + (size_t)Dj * r] = acc / Dj + (r == c ? 0.25 + 0.01 * (r % 7) : 0.0);
      }
  }

  vcmi_gmmmap g;      // host copies only: no device buffer is ever allocated
  HostModel hm;
  CHECK(factor_model(&g, hm, w.data(), mu.data(), sigma.data(), Dj, M, 0, px_only) == VCMI_OK);
  CHECK(hm.D == D && hm.DP == DP && hm.M == M && hm.px_only == px_only);
  const size_t pp = (size_t)DP * DP, reg = px_only ? 0 : 1;
  CHECK(hm.U.size() == pp * M && hm.cz.size() == (size_t)DP * M && hm.lc.size() == (size_t)M);
  CHECK(hm.A.size() == reg * pp * M && hm.b.size() == reg * DP * M);
  CHECK(g.h_mux.size() == (size_t)D * M && g.h_A.size() == reg * D * D * M);
  const bool tiles = gmmmap_has_mfma(DP), screen_rows = !px_only && D >= 4 && tiles && M <= 1024;
  CHECK(hm.P.size() == (screen_rows ? (size_t)M * 4 * DP : 0) && hm.cP.size() == (screen_rows ? (size_t)M * 4 : 0));

  if (!px_only) {
    const ModelProfile pf = profile_model(hm, g.h_mux, w.data());
    CHECK(pf.active >= 1.0 / M - 1e-12 && pf.active <= 1.0);      // a frame's best mixture always counts
    CHECK(pf.undecided >= pf.active - 1e-12 && pf.undecided <= 1.0);      // a lower bound of |z|^2 rules out no more than |z|^2
    for (int c = 0; c < 3; ++c) CHECK(pf.undecided_rows[c] >= (screen_rows ? pf.active - 1e-12 : 1.0) && pf.undecided_rows[c] <= 1.0);
    CHECK(pf.argmax_survivors > 0.0 && pf.argmax_survivors <= 1.0);
    if (screen_rows && screen_has_kernel(DP)) {
      const int rpm = choose_screen_rows(pf, DP, M);
      CHECK(rpm == 4 || rpm == 2 || rpm == 1);
    }
    CHECK(transpose_A(hm).size() == pp * M);
  }
  for (int variant = px_only ? 1 : 0; variant < 3 && tiles; ++variant) {
    const TilingRT tl(DP, variant != 0);
    int n = 0;
    for_each_fragment(tl, variant, [&](int t, int ks) { n += (t >= 0 && t < tl.NT && ks >= 0 && ks < tl.steps(t)); });
    CHECK(n == tl.NSTEPS);
    CHECK(pack_tiles(hm, variant).size() == (size_t)tl.BLK * M);
  }
  if (screen_rows) {
    for (int rpm = 1; rpm <= 4 && screen_has_kernel(DP); rpm *= 2)
      CHECK(pack_screen(hm, rpm).size() == (size_t)screen_stage_count(DP, M, rpm) * screen_stage_doubles(DP));
    if (screen_has_kernel(DP) && screen16_has(DP))
      CHECK(pack_screen_bf16(hm).size() == (size_t)screen_stage_count(DP, M, 4) * screen16_stage_doubles(DP));
    const std::vector<double> qa = pack_screen(hm, 4), ref = predict_screen(hm);
    CHECK(qa.size() == ref.size() && memcmp(qa.data(), ref.data(), qa.size() * sizeof(double)) == 0);
  }
  CHECK(pack_group_keys(hm, g.h_mux).size() == group_key_doubles(DP, M));
  CHECK(pack_group_keys_bf16(hm, g.h_mux).size() == group_key16_doubles(M));
}

int main() {
  run(7, 2, false);        // padding
  run(16, 3, false);       // one tile
  run(25, 4, false);       // padding across a tile edge
  run(40, 64, false);      // the headline shape, ten k-steps in the bf16 screen
  run(52, 5, false);       // two screen quads, no bf16 screen
  run(80, 8, false);       // widest tile kernel
  run(80, 4, true);        // widest tile kernel, p(x)-only
  run(160, 3, true);       // no tile kernel
  printf("prepare_check: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
