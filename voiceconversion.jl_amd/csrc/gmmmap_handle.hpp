// gmmmap_handle.hpp -- the opaque vcmi_gmmmap handle and the host functions around it (shared by the gmmmap*
// files, gmm_px_prep.hip, estep_full.hip, gmm_em.hip and the traj*.hip files).
#pragma once
#include "vcmi_common.hpp"
#include "gmmmap_layout.hpp"

namespace vcmi {
// What 256 frames drawn from the model itself say about it (sampled on the host by profile_model(), gmmmap_prepare.cpp, fixed
// seed): fractions of the M mixtures, means over the frames.
struct ModelProfile {
  // within e^-46 of the best one for the frame.  Reported by vcmi_gmmmap_convert_plan (synthetic SURVEY 8d models: 1/M; the
  // reference's trained 32-mixture model: 0.37).
  double active = 0.0;
  // ... that the LAST 16-row whitening tile's share of |z|^2 alone does not put e^-46 under the best one: what the "peaked"
  // loop's first test leaves undecided.  Selects the loop shape (convert_shape).
  double undecided = 0.0;
  // ... that the 4 / 2 / 1 strongest screening rows (largest eigenpairs of inv(Sxx_m)) leave undecided: what the screen of
  // shape 3 (gmmmap_screen.hpp) lets through with that many rows per mixture
  double undecided_rows[3] = {1.0, 1.0, 1.0};
  // ... whose four-row bound reaches the frame's best log-density: what predict's screen (gmmmap_screen_argmax_kernel) would
  // have to evaluate in full besides the frame's own mixture
  double argmax_survivors = 1.0;
  // the mixture every one of the 256 frames was drawn from and its exact |z|^2 there: what the group radius is judged on
  std::vector<int> own_m;
  std::vector<double> own_z2;
};

// The certified radius of every group for the screen of shape 3 (gmmmap_prepare.cpp: screen_radius_table, screen_radius_lmin;
// gmmmap_screen.hpp, step 1b).  For a group g, another mixture m, d = mu_m - mu_g and any lambda > 0, every x has
//   |z_m(x)|^2 + lambda |z_g(x)|^2 >= c_gm(lambda) = d' inv(Sxx_m + Sxx_g / lambda) d          (the minimum of a convex quadratic)
// so l_m(x) < l_g(x) - prune whenever |z_g(x)|^2 < (c_gm(lambda) - 2 (lc_m - lc_g + prune)) / (1 + lambda): weak duality, any
// lambda gives a valid radius, the grid only decides how sharp it is.  The table depends on the model alone and stays on the
// host; the radii follow from it for any prune without a factorisation.
struct ScreenRadius {
  static constexpr int J = 7;                         // lambda_j = 2^(j - 3): 1/8 .. 8, closed under 1 / lambda (c_mg(1 / lambda) = c_gm(lambda) / lambda)
  static constexpr int kMaxM = 128;                   // the cap: M^2 J doubles are 0.9 MB and M (M - 1) J / 2 = 57 k D x D factorisations there
  static double lambda(int j) { return (double)(1 << j) / 8.0; }
  int D = 0, M = 0;
  std::vector<double> c;                              // [M][M][J]; NaN: no bound (the diagonal, a factorisation that failed)
  std::vector<double> lc, mu_norm, l_norm;            // [M]: log-constants, |mu^x_m|, |L_m|_F (>= the longest half-axis of the unit ellipsoid)
  double u_norm = 0.0;                                // max over m of |U_m|_F
  bool empty() const { return c.empty(); }
};
}  // namespace vcmi

struct vcmi_gmmmap {
  int D = 0;    // dim(g): source feature dimension, src/gmmmap.jl:94
  int DP = 0;   // D rounded up to a multiple of 4 (MFMA k-step)
  int M = 0;    // ncomponents(g)
  int device = 0;
  int kernel_choice = 0;   // 0 auto, 1 generic VALU, 2 MFMA
  // fvconvert skips the regression of mixture m for a 16-frame tile when l_m < max_l - prune (nats) for all its frames:
  // the posterior there is below e^-prune (1e-20 at 46: under the rounding error of the sum).  +inf: dense loop.
  double prune = 46.0;
  vcmi::DevBuf<unsigned long long> prune_count;   // optional diagnostic counters (vcmi_gmmmap_prune_stats): [0] (tile, mixture) regressions, [1] FP64 MFMAs issued, [2] BF16 MFMAs of the screen, [3] workgroups that skipped the screen (group radius)
  vcmi::ModelProfile model;
  // rows per mixture of fvconvert's screen (choose_screen_rows(): the cheapest for this model) and what that many rows leave
  // undecided (model.undecided_rows): small (<= kScreenModelFrac) -> grouped calls run the screening kernel
  int screen_rpm = 4;
  double model_undecided4_frac = 1.0;
  // the group radius of shape 3 (ScreenRadius above): the host table, lmin[g] = lc_g - R_g / 2 on the device for the current
  // prune (+inf: nothing is certified for g), the share of the model's own 256 frames inside their mixture's radius and
  // whether the kernel looks at lmin at all (decided once, at creation: choose_screen_radius)
  vcmi::ScreenRadius radius;
  vcmi::DevBuf<double> lmin;
  double radius_pass_frac = 0.0;
  bool radius_on = false;

  // host copies kept for accessors and for TrajectoryGMMMap's constructor (row-major (D,D) per mixture)
  std::vector<double> h_A_julia;   // Julia memory image (D,D,M) of ΣʸˣΣˣˣ⁻¹
  std::vector<double> h_A, h_Sxy, h_Syy, h_mux, h_muy;

  // device parameters, generic layout: [M][DP][DP] row-major / [M][DP] / [M]
  vcmi::DevBuf<double> U, A, cz, b, lc;
  vcmi::DevBuf<double> At;        // A transposed, [M][DP (k)][DP (row)]: only for dimensions without a tile-kernel instantiation
  // device parameters, MFMA fragment order: [M][Tiling::BLK]
  vcmi::DevBuf<double> packed;    // [U_m ; A_m] tiles (convert)
  vcmi::DevBuf<double> packedU;   // U_m tiles only (log-density / posterior / argmax)
  vcmi::DevBuf<double> packedQ;   // stages of the screen: 4 tiles x (screen_rpm rows of 16 / screen_rpm mixtures) per stage (convert, shape 3)
  vcmi::DevBuf<double> packedQ16;  // the four-row screen split into bf16 hi + lo (screen on the BF16 matrix pipe; DP <= 40)
  vcmi::DevBuf<double> packedQ2;   // sixteen rows per mixture, one tile each: the second look of that screen (uploaded with packedQ16)
  vcmi::DevBuf<double> packedQA;  // stages of predict's screen: four rows per mixture, every tile-kernel dimension (gmmmap_screen_argmax_kernel)
  vcmi::DevBuf<double> packedU2;  // U_m tiles only, tile by tile, last tile first (predict with early exit; host-prepared handles)
  // fvconvert's frame grouping (gmmmap_group_key_kernel): nearest-source-mean operand [-2 mu | |mu|^2] in MFMA fragment order,
  // and the call's scratch: key (T), perm (T), counts (M), cursors (M)
  vcmi::DevBuf<double> gfrag;
  vcmi::DevBuf<double> gfrag16;   // the same operand split into bf16 hi + lo for gmmmap_group_key16_kernel
  // grp: key (T), perm (T), the chunk histograms (nchunks, M) and gbase (M + 1): the first sorted position of every group, gbase[M] = T
  vcmi::DevBuf<int> grp;
  vcmi::StreamOrder grp_order;   // orders every call that uses the handle's scratch: grp, grp_super and scratch_lp below
  // the grouping's super-chunk histograms: TWO tables of grp_super_stride ints, each all zero between the calls that use it
  // (launch_grouping, gmmmap_group.hip: call n adds into table n & 1 and clears the other one).  grp_super_used[i]: ints of table i
  // that the last call on it left non-zero; grp_super_ok: false until the tables are known to be in that state (new or grown
  // buffer, a call whose launches did not all go out) -- the next call then zeroes both before it starts.
  vcmi::DevBuf<int> grp_super;
  size_t grp_super_stride = 0;
  size_t grp_super_used[2] = {0, 0};
  unsigned grp_calls = 0;
  bool grp_super_ok = false;
  int cus = 256;   // compute units of `device` (bind_device)
  void bind_device(int dev) {
    device = dev;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
  }

  // issue-order table of the U-only tiling (slot -> tile << 16 | k-step) for the on-device packer (gmm_px_prepare_device)
  vcmi::DevBuf<int> px_table;
  int px_table_dp = 0;

  // grow-only device scratch (two-pass predict of the generic path, fvconvert of 80 < D <= 160), under grp_order
  vcmi::DevBuf<double> scratch_lp;

  // constructor arguments, kept so that the converter can be re-created on the other devices of a device group
  // (vcmi_set_devices): replicas[i] lives on member i's device and is made lazily by that member's worker thread
  std::vector<double> in_w, in_mu, in_sigma;
  int in_Dj = 0, in_swap = 0;
  std::vector<vcmi_gmmmap *> replicas;
  uint64_t replicas_epoch = 0;
  ~vcmi_gmmmap() {
    for (vcmi_gmmmap *r : replicas) delete r;
  }
};

namespace vcmi {
// Host-side preparation (gmmmap_prepare.cpp): factorises the joint GMM (weights (M), mu (Dj,M), sigma (Dj,Dj,M), Julia
// memory images), profiles it, and packs and uploads every device image of g on the current device.
// px_only: (mu, sigma) describe a plain GMM p(x) of dimension Dj (no target half): only the whitening side is prepared
// (used by the full-covariance E-step, estep_full.hip); the regression blocks stay zero and the convert layouts are skipped.
int gmmmap_prepare(vcmi_gmmmap *g, const double *w, const double *mu, const double *sigma, int Dj, int M, int swap,
                   bool px_only = false);
// *inout becomes a handle on the current device: the existing one if it lives there, else a new one (the old one deleted)
int gmm_px_handle_here(vcmi_gmmmap **inout);
// p(x)-only handle over a plain GMM of dimension D (weights (M), mu (D,M), sigma (D,D,M)); used by estep_full.hip and gmm_em.hip.
// *out == nullptr creates a handle; otherwise the existing handle (same device) is re-prepared in place, reusing its
// device buffers -- the caller must have drained every stream that still reads them.
int gmm_px_create(const double *w, const double *mu, const double *sigma, int D, int M, vcmi_gmmmap **out);
// Same handle prepared ON THE DEVICE from device-resident parameters (w (M), mu (D,M), sigma (D,D,M)): one workgroup
// per mixture does the Cholesky, the triangular inverse and the MFMA operand packing.  Asynchronous on `st`;
// *d_flag (device int, zeroed by the caller) receives m+1 for a mixture whose covariance is not positive definite.
// (gmm_px_prep.hip)
bool gmm_px_device_prepare_supported(int D);
int gmm_px_prepare_device(vcmi_gmmmap **inout, const double *d_w, const double *d_mu, const double *d_sigma, int D, int M,
                          int *d_flag, hipStream_t st);
// The device routines behind the C entry points (gmmmap.hip): device pointers, asynchronous on st.
int gmmmap_convert_device(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy, hipStream_t st);
int gmmmap_logdens_device(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dLP, hipStream_t st);
int gmmmap_posterior_device(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dP, hipStream_t st);
// allow_screen: long inputs may be grouped and run the screened arg-max (exact; pays for draws from a peaked p(x))
int gmmmap_predict_device(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, int64_t *didx, hipStream_t st, bool allow_screen = true);
// vcmi_gmmmap_convert_plan's shape: -1 no tile kernel for g, 0 dense (prune = +inf), 1 broad, 2 peaked, 3 screened
int gmmmap_convert_plan_shape(const vcmi_gmmmap *g);
// lmin of g->radius for g->prune -> g->lmin on the current device (gmmmap_prepare.cpp); waits for the handle's last grouped
// call, whose kernel may still read the buffer.  Nothing to do for a handle without a table.
int screen_radius_upload(vcmi_gmmmap *g);
// Device group support (devgroup.hpp, gmmmap_api.cpp): gmmmap_sync_replicas is called by the host thread before group_run; inside the
// run member i obtains its converter (g itself on g's device, else a replica created on first use).
void gmmmap_sync_replicas(vcmi_gmmmap *g);
int gmmmap_member(vcmi_gmmmap *g, int member, vcmi_gmmmap **out);
}  // namespace vcmi
