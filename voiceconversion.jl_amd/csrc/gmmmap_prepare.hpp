// gmmmap_prepare.hpp -- the steps of gmmmap_prepare() (gmmmap_handle.hpp), each a host function of its own: factor the
// model, profile it, choose the screen's rows, pack the device images.  Only factor_model() touches a handle (its host
// copies); nothing here touches the device, so the steps also run in the CPU sanitizer build (tests/c/prepare_check.cpp).
#pragma once
#include <vector>
#include "gmmmap_handle.hpp"

namespace vcmi {

// Row-major host images of a factored model, rows and columns padded with zeros to DP.
struct HostModel {
  int D = 0, DP = 0, M = 0;
  bool px_only = false;             // p(x) only: A and b are empty
  std::vector<double> U, A;         // [M][DP][DP]
  std::vector<double> cz, b;        // [M][DP]
  std::vector<double> lc;           // [M]
  std::vector<double> P, cP;        // screening rows [M][4][DP], strongest first, and their constants [M][4]; empty: no screen
  std::vector<double> P2, cP2;      // the min(16, D) strongest rows [M][16][DP] and constants [M][16]: rows 0..3 are P's, missing rows zero; empty unless screen16_has(DP)
  std::vector<double> Sxx;          // Hermitian(Sxx_m), [M][D][D] (not padded): only where the group radius is computed (screen, M <= ScreenRadius::kMaxM)
};
// Fills hm and g's host copies (h_A_julia, h_A, h_Sxy, h_Syy, h_mux, h_muy) from the joint GMM; VCMI_ERR_NOT_PD names the
// first mixture whose Sigma^xx cannot be factored.
int factor_model(vcmi_gmmmap *g, HostModel &hm, const double *w, const double *mu, const double *sigma, int Dj, int M, int swap,
                 bool px_only);

// ModelProfile: gmmmap_handle.hpp
ModelProfile profile_model(const HostModel &hm, const std::vector<double> &mux, const double *w);
// rows per mixture (4, 2 or 1) of fvconvert's screen with the smallest estimated cost per 16-frame tile
int choose_screen_rows(const ModelProfile &pf, int DP, int M);

// The group radius of shape 3 (ScreenRadius, gmmmap_handle.hpp).  The table: one Cholesky factorisation of Sxx_m + Sxx_g / lambda_j
// and one forward substitution per unordered pair and lambda, shared out over the library's host threads.  hm.Sxx must be there.
ScreenRadius screen_radius_table(const HostModel &hm, const std::vector<double> &mux);
// R[g] (M; the certified radius of |z_g|^2 less the rounding margin; <= 0 or -inf: none) and lmin[g] = lc_g - R[g] / 2 (+inf: none)
// for one prune.  No factorisation: a minimum over the table.
void screen_radius_lmin(const ScreenRadius &rt, double prune, std::vector<double> &R, std::vector<double> &lmin);
// share of the profile's own frames that lie inside their mixture's radius, and the rule on it: choose_screen_radius
double screen_radius_pass_frac(const ModelProfile &pf, const ScreenRadius &rt, const std::vector<double> &lmin);
bool choose_screen_radius(double pass_frac);

// The device images (gmmmap_handle.hpp names them; gmmmap_layout.hpp gives their layouts and lengths).
std::vector<double> pack_tiles(const HostModel &hm, int variant);    // packed (0), packedU (1), packedU2 (2): for_each_fragment's variants
std::vector<double> pack_screen(const HostModel &hm, int rpm);       // packedQ; rpm = 4: packedQA
std::vector<double> pack_screen_bf16(const HostModel &hm);           // packedQ16 (four rows per mixture)
std::vector<double> pack_screen2_bf16(const HostModel &hm);          // packedQ2 (sixteen rows per mixture: the second look)
std::vector<double> pack_group_keys(const HostModel &hm, const std::vector<double> &mux);        // gfrag
std::vector<double> pack_group_keys_bf16(const HostModel &hm, const std::vector<double> &mux);   // gfrag16
std::vector<double> transpose_A(const HostModel &hm);                // At

}  // namespace vcmi
