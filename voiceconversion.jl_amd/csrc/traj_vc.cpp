// traj_vc.cpp -- vc of a trajectory converter (reference bin/vc.jl:75-82, src/common.jl:31-63, src/gv.jl:10-15): vcmi_vc_traj on
// the host-batch path; with the post-filter, from STATIC features, on device matrices or with the GV ascent (vcmi_vc_traj_postf,
// vcmi_vc_traj_static, vcmi_vc_trajgv, vcmi_vc_traj_dev, vcmi_vc_trajgv_dev) through vc_traj_device.  Nothing here launches a
// kernel: the chunks go through traj_run (traj.hip), the two ends through the routines of postf.hpp.
#include "traj_internal.hpp"
#include "hostpipe.hpp"
#include "postf.hpp"

#include <algorithm>

using namespace vcmi;

namespace vcmi {

// the checks of a call with T > 0 frames, and its chunk lengths [kL+1, min((k+1)L, T)], src/common.jl:42-57
static int vc_traj_args(const vcmi_traj *t, const vcmi_trajgv *gvh, int epochs, int64_t T, const double *sigma2,
                        std::vector<int64_t> &Ts, TrajGV *gv, const char *who) {
  if (sigma2 && T < 2) return fail(VCMI_ERR_DIM, "%s: the variance of a one-frame matrix is undefined", who);
  if (t->length < 1) return fail(VCMI_ERR_ARG, "%s: length(t) must be positive", who);
  const int64_t L = t->length, nch = (T + L - 1) / L;
  if (std::min(L, T) > INT32_MAX) return fail(VCMI_ERR_DIM, "%s: bad chunk length", who);
  Ts.resize((size_t)nch);
  for (int64_t k = 0; k < nch; ++k) Ts[(size_t)k] = std::min<int64_t>(L, T - k * L);
  if (gvh) VCMI_TRY(trajgv_args(gvh, nch, Ts.data(), epochs, gv));      // a one-frame chunk has no variance: VCMI_ERR_DIM
  return VCMI_OK;
}

// The one routine behind the five entries.  dfm (D+1,T) static or (dim(t)+1,T), dim(t) = 2D (3D with three windows); dout (D+1,T); gvh != NULL: every chunk through
// fvconvert(tgv, X; epochs, alpha).  dout == dfm (static input only) assembles the result in place: the power row never
// moves, rows 2..D+1 are overwritten after the pre kernel has read them.  Every argument is checked before the first launch.
static int vc_traj_device(vcmi_traj *t, vcmi_trajgv *gvh, int epochs, double alpha, const double *dfm, int64_t ldf, int64_t T,
                          bool is_static, const double *sigma2, double *dout, int64_t ldo, hipStream_t st, const char *who) {
  if (T < 0 || (T > 0 && (!dfm || !dout))) return fail(VCMI_ERR_ARG, "%s: bad argument", who);
  if (is_static) VCMI_TRY(traj_two_windows_only(t, who, "static input (the deltas taken by the library)"));
  if (T == 0) return VCMI_OK;
  const int D = t->D, D2 = t->D2, rows = (is_static ? D : D2) + 1;
  if (ldf < rows || ldo < D + 1) return fail(VCMI_ERR_ARG, "%s: leading dimension below the row count", who);
  std::vector<int64_t> Ts;
  TrajGV gv{};
  gv.alpha = alpha;
  VCMI_TRY(vc_traj_args(t, gvh, epochs, T, sigma2, Ts, &gv, who));
  const int64_t L = t->length, nch = (int64_t)Ts.size();
  std::vector<TrajUtt> utts((size_t)nch);
  VCMI_TRY(check_device());
  VcScratch &sc = vc_scratch();
  TrajEmRelease em_release{t};
  VCMI_TRY(sc.x.reserve((size_t)D2 * T));
  VCMI_TRY(sc.y.reserve((size_t)D * T));
  VCMI_TRY(sc.order.enter(st));
  // X = [fm[1,:]; push_delta(fm[2:end,:])] over the whole matrix (bin/vc.jl:77-78), or rows 2..dim(t)+1 as they are
  VCMI_TRY(vc_traj_pre_device(dfm, ldf, D, D2, T, is_static, sc.x.p, dout == dfm ? nullptr : dout, ldo, st));
  for (int64_t k = 0; k < nch; ++k)
    utts[(size_t)k] = TrajUtt{sc.x.p + (size_t)k * L * D2, sc.y.p + (size_t)k * L * D, k * L, (int32_t)Ts[(size_t)k], (int32_t)k};
  VCMI_TRY(traj_run(t, utts, T, true, sc.x.p, st, gvh ? &gv : nullptr));
  const double *stat = nullptr;
  if (sigma2) VCMI_TRY(variance_scaling_stats_device(sc.y.p, D, D, T, sigma2, &stat, st));   // fvpostf! over all T frames
  VCMI_TRY(vc_traj_post_device(sc.y.p, D, T, stat, dout, ldo, st));
  if (sigma2) VCMI_TRY(variance_scaling_stats_leave(st));
  VCMI_TRY(sc.order.leave(st));
  VCMI_TRY(traj_check_status(t, st));
  t->length = Ts[(size_t)nch - 1];   // as vcmi_vc_traj: the last fvconvert of the loop left W at the last chunk's length
  return VCMI_OK;
}

// host-pointer form: staged_upload -> vc_traj_device -> staged_download.  Static input is assembled in place in the staging
// matrix (out has the shape of fm); the (2D+1,T) input gets its (D+1,T) result behind it in the same buffer.
static int vc_traj_host(vcmi_traj *t, vcmi_trajgv *gvh, int epochs, double alpha, const double *fm, int64_t T, bool is_static,
                        const double *sigma2, double *out, const char *who) {
  if (T < 0 || (T > 0 && (!fm || !out))) return fail(VCMI_ERR_ARG, "%s: bad argument", who);
  if (is_static) VCMI_TRY(traj_two_windows_only(t, who, "static input (the deltas taken by the library)"));
  if (T == 0) return VCMI_OK;
  {   // nothing is uploaded for a call that cannot run
    std::vector<int64_t> Ts;
    TrajGV gv{};
    VCMI_TRY(vc_traj_args(t, gvh, epochs, T, sigma2, Ts, &gv, who));
  }
  VCMI_TRY(check_device());
  VcScratch &sc = vc_scratch();
  VcScratch::Release release{sc};   // on every way out
  const int D = t->D, rows = (is_static ? D : t->D2) + 1;
  const size_t nin = (size_t)rows * T, nout = (size_t)(D + 1) * T;
  VCMI_TRY(sc.stage.reserve(is_static ? nin : nin + nout));
  double *dout = is_static ? sc.stage.p : sc.stage.p + nin;
  VCMI_TRY(staged_upload(sc.stage.p, fm, sizeof(double) * nin, nullptr));
  VCMI_TRY(vc_traj_device(t, gvh, epochs, alpha, sc.stage.p, rows, T, is_static, sigma2, dout, D + 1, nullptr, who));
  return staged_download(out, dout, sizeof(double) * nout, nullptr);
}

}  // namespace vcmi

extern "C" int vcmi_vc_traj(vcmi_traj *t, const double *fm, int64_t T, double *out) {
  if (!t) return fail(VCMI_ERR_ARG, "vcmi_vc_traj: NULL handle");
  if (T < 0 || (T > 0 && (!fm || !out))) return fail(VCMI_ERR_ARG, "vcmi_vc_traj: bad argument");
  if (T == 0) return VCMI_OK;
  std::vector<int64_t> Ts;
  VCMI_TRY(vc_traj_args(t, nullptr, 0, T, nullptr, Ts, nullptr, "vcmi_vc_traj"));
  const int D = t->D, D2 = t->D2;
  const int64_t L = t->length, nch = (int64_t)Ts.size();
  std::vector<double> x((size_t)T * D2), y((size_t)T * D);
  for (int64_t f = 0; f < T; ++f) memcpy(&x[(size_t)f * D2], fm + (size_t)f * (D2 + 1) + 1, sizeof(double) * D2);
  std::vector<const double *> xs(nch);
  std::vector<double *> ys(nch);
  for (int64_t k = 0; k < nch; ++k) {
    xs[k] = &x[(size_t)k * L * D2];
    ys[k] = &y[(size_t)k * L * D];
  }
  VCMI_TRY(traj_host_batch(t, nch, xs.data(), Ts.data(), ys.data()));
  for (int64_t f = 0; f < T; ++f) {
    out[(size_t)f * (D + 1)] = fm[(size_t)f * (D2 + 1)];   // power row kept, src/common.jl:60
    memcpy(out + (size_t)f * (D + 1) + 1, &y[(size_t)f * D], sizeof(double) * D);
  }
  t->length = Ts[nch - 1];   // the last fvconvert of the loop left W at the last chunk's length (see vcmi_traj_convert)
  return VCMI_OK;
}

// vc(c::TrajectoryConverter, fm) followed by fvpostf!(VarianceScaling(sigma2), converted[2:end, :]) -- src/common.jl:31-63,
// src/gv.jl:10-15 -- with the matrix resident in HBM from the upload of fm to the download of the filtered result.  Without a
// filter the call is vcmi_vc_traj's (device group, bounded pinned ring).
extern "C" int vcmi_vc_traj_postf(vcmi_traj *t, const double *fm, int64_t T, const double *sigma2, double *out) {
  if (!sigma2) return vcmi_vc_traj(t, fm, T, out);
  if (!t) return fail(VCMI_ERR_ARG, "vcmi_vc_traj_postf: NULL handle");
  return vc_traj_host(t, nullptr, 0, 0.0, fm, T, false, sigma2, out, "vcmi_vc_traj_postf");
}

extern "C" int vcmi_vc_traj_static(vcmi_traj *t, const double *fm, int64_t T, const double *sigma2, double *out) {
  if (!t) return fail(VCMI_ERR_ARG, "vcmi_vc_traj_static: NULL handle");
  return vc_traj_host(t, nullptr, 0, 0.0, fm, T, true, sigma2, out, "vcmi_vc_traj_static");
}

extern "C" int vcmi_vc_trajgv(vcmi_trajgv *h, const double *fm, int64_t T, int is_static, int epochs, double alpha,
                              const double *sigma2, double *out) {
  if (!h) return fail(VCMI_ERR_ARG, "vcmi_vc_trajgv: NULL handle");
  return vc_traj_host(h->t, h, epochs, alpha, fm, T, is_static != 0, sigma2, out, "vcmi_vc_trajgv");
}

extern "C" int vcmi_vc_traj_dev(vcmi_traj *t, const double *dfm, int64_t ldf, int64_t T, int is_static, const double *sigma2,
                                double *dout, int64_t ldo, void *stream) {
  if (!t) return fail(VCMI_ERR_ARG, "vcmi_vc_traj_dev: NULL handle");
  if (dfm && dfm == dout) return fail(VCMI_ERR_ARG, "vcmi_vc_traj_dev: dout must not overlap dfm");
  return vc_traj_device(t, nullptr, 0, 0.0, dfm, ldf, T, is_static != 0, sigma2, dout, ldo, as_stream(stream), "vcmi_vc_traj_dev");
}

extern "C" int vcmi_vc_trajgv_dev(vcmi_trajgv *h, const double *dfm, int64_t ldf, int64_t T, int is_static, int epochs,
                                  double alpha, const double *sigma2, double *dout, int64_t ldo, void *stream) {
  if (!h) return fail(VCMI_ERR_ARG, "vcmi_vc_trajgv_dev: NULL handle");
  if (dfm && dfm == dout) return fail(VCMI_ERR_ARG, "vcmi_vc_trajgv_dev: dout must not overlap dfm");
  return vc_traj_device(h->t, h, epochs, alpha, dfm, ldf, T, is_static != 0, sigma2, dout, ldo, as_stream(stream),
                        "vcmi_vc_trajgv_dev");
}
