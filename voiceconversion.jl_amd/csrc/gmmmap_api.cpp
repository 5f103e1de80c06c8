// gmmmap_api.cpp -- the C entry points of the converter (vcmi_gmmmap_*, vcmi_vc_frames) and what only they need: the
// device-group replicas and the split of a call's frames over the group.  Host code only (no kernel lives here, so an edit
// does not recompile one); the device routines it calls are those gmmmap_handle.hpp declares.
#include "vcmi_common.hpp"
#include "gmmmap_handle.hpp"
#include "devgroup.hpp"
#include "hostpipe.hpp"

#include <cmath>

// ------------------------------------------------------------------------------------------------
// device-group replicas (devgroup.hpp)
// ------------------------------------------------------------------------------------------------
namespace vcmi {

void gmmmap_sync_replicas(vcmi_gmmmap *g) {
  const uint64_t ep = group_epoch();
  if (g->replicas_epoch == ep && (int)g->replicas.size() == group_size()) return;
  for (vcmi_gmmmap *r : g->replicas) delete r;
  g->replicas.assign((size_t)group_size(), nullptr);
  g->replicas_epoch = ep;
}

int gmmmap_member(vcmi_gmmmap *g, int member, vcmi_gmmmap **out) {
  // g itself serves the first member that sits on g's device; every other member gets its own converter
  bool first_on_home = group_device(member) == g->device;
  for (int k = 0; k < member && first_on_home; ++k)
    if (group_device(k) == g->device) first_on_home = false;
  if (first_on_home) {
    *out = g;
    return VCMI_OK;
  }
  vcmi_gmmmap *&r = g->replicas[(size_t)member];
  if (!r) {
    if (g->in_w.empty()) return fail(VCMI_ERR_ARG, "this converter cannot be replicated on another device");
    vcmi_gmmmap *n = new (std::nothrow) vcmi_gmmmap();
    if (!n) return fail(VCMI_ERR_OOM, "out of host memory");
    int ndev = 0;
    (void)hipGetDevice(&ndev);
    n->bind_device(ndev);
    const int rc = gmmmap_prepare(n, g->in_w.data(), g->in_mu.data(), g->in_sigma.data(), g->in_Dj, g->M, g->in_swap);
    if (rc != VCMI_OK) {
      delete n;
      return rc;
    }
    r = n;
  }
  r->kernel_choice = g->kernel_choice;
  if (r->prune != g->prune) {
    r->prune = g->prune;
    VCMI_TRY(screen_radius_upload(r));           // (on the member's device: this runs on its worker thread)
  }
  *out = r;
  return VCMI_OK;
}

// frames below which a call is not worth spreading over the group
static constexpr int64_t kGroupMinFrames = 4096;
// chunks of the host pipeline hold at least this many frames: one full round of workgroups on 256 CUs
static constexpr int64_t kMinChunkFrames = 98304;

// Frames are independent: member i of the group converts the contiguous block [lo, hi).
template <class PerShard>
static int over_frames(vcmi_gmmmap *g, int64_t T, const PerShard &fn) {
  const int m = group_size();
  if (m == 0 || T < kGroupMinFrames) return fn(g, (int64_t)0, T);
  gmmmap_sync_replicas(g);
  return group_run(m, [&](int i) -> int {
    int64_t lo, hi;
    shard_range(T, i, m, &lo, &hi);
    if (hi == lo) return VCMI_OK;
    vcmi_gmmmap *r = nullptr;
    VCMI_TRY(gmmmap_member(g, i, &r));
    return fn(r, lo, hi);
  });
}

}  // namespace vcmi

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
using namespace vcmi;

extern "C" int vcmi_gmmmap_create(const double *weights, const double *mu, const double *sigma, int Dj, int M, int swap,
                                  vcmi_gmmmap **out) {
  if (!weights || !mu || !sigma || !out) return fail(VCMI_ERR_ARG, "vcmi_gmmmap_create: NULL argument");
  if (Dj < 2 || (Dj & 1) || M < 1) return fail(VCMI_ERR_DIM, "vcmi_gmmmap_create: joint dimension %d / mixtures %d invalid", Dj, M);
  *out = nullptr;
  VCMI_TRY(check_device());
  vcmi_gmmmap *g = new (std::nothrow) vcmi_gmmmap();
  if (!g) return fail(VCMI_ERR_OOM, "out of host memory");
  int dev = 0;
  (void)hipGetDevice(&dev);
  g->bind_device(dev);
  int rc = gmmmap_prepare(g, weights, mu, sigma, Dj, M, swap);
  if (rc != VCMI_OK) {
    delete g;
    return rc;
  }
  g->in_w.assign(weights, weights + M);
  g->in_mu.assign(mu, mu + (size_t)Dj * M);
  g->in_sigma.assign(sigma, sigma + (size_t)Dj * Dj * M);
  g->in_Dj = Dj;
  g->in_swap = swap;
  *out = g;
  return VCMI_OK;
}

extern "C" int vcmi_gmmmap_destroy(vcmi_gmmmap *g) {
  delete g;
  return VCMI_OK;
}
extern "C" int vcmi_gmmmap_dim(const vcmi_gmmmap *g) { return g ? g->D : -1; }
extern "C" int vcmi_gmmmap_ncomponents(const vcmi_gmmmap *g) { return g ? g->M : -1; }
extern "C" int vcmi_gmmmap_get_A(const vcmi_gmmmap *g, double *A) {
  if (!g || !A) return fail(VCMI_ERR_ARG, "vcmi_gmmmap_get_A: NULL argument");
  memcpy(A, g->h_A_julia.data(), g->h_A_julia.size() * sizeof(double));
  return VCMI_OK;
}
extern "C" int vcmi_gmmmap_set_kernel(vcmi_gmmmap *g, int which) {
  if (!g || which < 0 || which > 2) return fail(VCMI_ERR_ARG, "vcmi_gmmmap_set_kernel: bad argument");
  if (which == 2 && !gmmmap_has_mfma(g->DP)) return fail(VCMI_ERR_ARG, "no MFMA instantiation for dimension %d", g->D);
  g->kernel_choice = which;
  return VCMI_OK;
}

extern "C" int vcmi_gmmmap_prune_stats(vcmi_gmmmap *g, int enable, int64_t *evaluated) {
  if (!g) return fail(VCMI_ERR_ARG, "vcmi_gmmmap_prune_stats: NULL handle");
  if (evaluated) {
    *evaluated = 0;
    if (g->prune_count.p) {
      unsigned long long h = 0;
      VCMI_HIP(hipMemcpy(&h, g->prune_count.p, sizeof(h), hipMemcpyDeviceToHost));     // (synchronises with the null stream)
      *evaluated = (int64_t)h;
    }
  }
  if (enable) {
    if (!g->prune_count.p) VCMI_TRY(g->prune_count.alloc(4));
    VCMI_HIP(hipMemset(g->prune_count.p, 0, 4 * sizeof(unsigned long long)));
  } else {
    g->prune_count.release();
  }
  return VCMI_OK;
}

extern "C" int vcmi_gmmmap_convert_plan(vcmi_gmmmap *g, int64_t *mfma_issued, int *shape, double *model_active_frac,
                                        double *model_undecided_frac) {
  if (!g) return fail(VCMI_ERR_ARG, "vcmi_gmmmap_convert_plan: NULL handle");
  if (mfma_issued) {
    *mfma_issued = 0;
    if (g->prune_count.p) {
      unsigned long long h = 0;
      VCMI_HIP(hipMemcpy(&h, g->prune_count.p + 1, sizeof(h), hipMemcpyDeviceToHost));
      *mfma_issued = (int64_t)h;
    }
  }
  if (shape) *shape = gmmmap_convert_plan_shape(g);
  if (model_active_frac) *model_active_frac = g->model.active;
  if (model_undecided_frac) *model_undecided_frac = g->model.undecided;
  return VCMI_OK;
}

extern "C" int vcmi_gmmmap_set_prune(vcmi_gmmmap *g, double nats) {
  if (!g) return fail(VCMI_ERR_ARG, "vcmi_gmmmap_set_prune: NULL handle");
  if (!(nats >= 40.0)) return fail(VCMI_ERR_ARG, "vcmi_gmmmap_set_prune: threshold %g nats would change y at double precision (>= 40)", nats);
  const double prune = nats >= 1e300 ? INFINITY : nats;
  if (prune == g->prune) return VCMI_OK;
  g->prune = prune;
  // the group radii of shape 3 depend on it: lmin again from the host table (no factorisation), on the handle's device
  if (g->radius.empty()) return VCMI_OK;
  int dev = 0;
  VCMI_HIP(hipGetDevice(&dev));
  if (dev != g->device) VCMI_HIP(hipSetDevice(g->device));
  const int rc = screen_radius_upload(g);
  if (dev != g->device) VCMI_HIP(hipSetDevice(dev));
  return rc;
}

extern "C" int vcmi_gmmmap_screen_radius_stats(vcmi_gmmmap *g, int64_t *skipped, int *in_use, double *pass_frac) {
  if (!g) return fail(VCMI_ERR_ARG, "vcmi_gmmmap_screen_radius_stats: NULL handle");
  if (skipped) {
    *skipped = 0;
    if (g->prune_count.p) {
      unsigned long long h = 0;
      VCMI_HIP(hipMemcpy(&h, g->prune_count.p + 3, sizeof(h), hipMemcpyDeviceToHost));
      *skipped = (int64_t)h;
    }
  }
  if (in_use) *in_use = g->radius_on ? 1 : 0;
  if (pass_frac) *pass_frac = g->radius_pass_frac;
  return VCMI_OK;
}

static int check_xy(const vcmi_gmmmap *g, const void *X, int64_t ldx, int64_t T, const void *Y, int64_t ldy, const char *who) {
  if (!g) return fail(VCMI_ERR_ARG, "%s: NULL handle", who);
  if (T < 0) return fail(VCMI_ERR_ARG, "%s: negative frame count", who);
  if (T > 0 && (!X || !Y)) return fail(VCMI_ERR_ARG, "%s: NULL buffer", who);
  if (ldx < g->D || ldy < 1) return fail(VCMI_ERR_DIM, "%s: Inconsistent dimensions (leading dimension %lld < dim %d)", who, (long long)ldx, g->D);
  return VCMI_OK;
}

extern "C" int vcmi_gmmmap_convert_dev(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy,
                                       void *stream) {
  VCMI_TRY(check_xy(g, dX, ldx, T, dY, ldy, "vcmi_gmmmap_convert_dev"));
  if (ldy < g->D) return fail(VCMI_ERR_DIM, "vcmi_gmmmap_convert_dev: ldy %lld < dim %d", (long long)ldy, g->D);
  return gmmmap_convert_device(g, dX, ldx, T, dY, ldy, as_stream(stream));
}

// Host pointers: chunks of frames travel pageable -> pinned -> HBM -> kernel -> pinned -> pageable with the three
// stages of consecutive chunks overlapping (hostpipe.hpp); with a device group the frame range is split first.
extern "C" int vcmi_gmmmap_convert(vcmi_gmmmap *g, const double *X, int64_t ldx, int64_t T, double *Y, int64_t ldy) {
  VCMI_TRY(check_xy(g, X, ldx, T, Y, ldy, "vcmi_gmmmap_convert"));
  if (ldy < g->D) return fail(VCMI_ERR_DIM, "vcmi_gmmmap_convert: ldy %lld < dim %d", (long long)ldy, g->D);
  if (T == 0) return VCMI_OK;
  const size_t row = (size_t)g->D * 8;
  return over_frames(g, T, [&](vcmi_gmmmap *r, int64_t lo, int64_t hi) -> int {
    return staged_pipeline(X + lo * ldx, row, (size_t)ldx * 8, Y + lo * ldy, row, (size_t)ldy * 8, hi - lo, kMinChunkFrames,
                           [&](const void *dIn, void *dOut, int64_t, int64_t n, hipStream_t st) -> int {
                             return gmmmap_convert_device(r, (const double *)dIn, r->D, n, (double *)dOut, r->D, st);
                           });
  });
}

extern "C" int vcmi_vc_frames(vcmi_gmmmap *g, const double *fm, int64_t T, double *out) {
  if (!g) return fail(VCMI_ERR_ARG, "vcmi_vc_frames: NULL handle");
  if (T < 0 || (T > 0 && (!fm || !out))) return fail(VCMI_ERR_ARG, "vcmi_vc_frames: bad argument");
  if (T == 0) return VCMI_OK;
  const int64_t ld = g->D + 1;   // row 1 is the power coefficient, src/common.jl:11
  const size_t row = (size_t)ld * 8;
  return over_frames(g, T, [&](vcmi_gmmmap *r, int64_t lo, int64_t hi) -> int {
    return staged_pipeline(fm + lo * ld, row, row, out + lo * ld, row, row, hi - lo, kMinChunkFrames,
                           [&](const void *dIn, void *dOut, int64_t, int64_t n, hipStream_t st) -> int {
                             // the copy keeps row 1 (src/common.jl:23); the kernel then overwrites rows 2..D+1
                             // (hipMemcpyDefault: a small call hands the pinned slots themselves to this function)
                             VCMI_HIP(hipMemcpyAsync(dOut, dIn, (size_t)n * row, hipMemcpyDefault, st));
                             return gmmmap_convert_device(r, (const double *)dIn + 1, ld, n, (double *)dOut + 1, ld, st);
                           });
  });
}

extern "C" int vcmi_gmmmap_posterior_dev(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dP, void *stream) {
  VCMI_TRY(check_xy(g, dX, ldx, T, dP, 1, "vcmi_gmmmap_posterior_dev"));
  return gmmmap_posterior_device(g, dX, ldx, T, dP, as_stream(stream));
}

extern "C" int vcmi_gmmmap_posterior(vcmi_gmmmap *g, const double *X, int64_t ldx, int64_t T, double *P) {
  VCMI_TRY(check_xy(g, X, ldx, T, P, 1, "vcmi_gmmmap_posterior"));
  if (T == 0) return VCMI_OK;
  const int M = g->M;
  return over_frames(g, T, [&](vcmi_gmmmap *r, int64_t lo, int64_t hi) -> int {
    return staged_pipeline(X + lo * ldx, (size_t)r->D * 8, (size_t)ldx * 8, P + lo * M, (size_t)M * 8, (size_t)M * 8, hi - lo,
                           kMinChunkFrames, [&](const void *dIn, void *dOut, int64_t, int64_t n, hipStream_t st) -> int {
                             return gmmmap_posterior_device(r, (const double *)dIn, r->D, n, (double *)dOut, st);
                           });
  });
}

extern "C" int vcmi_gmmmap_predict_dev(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, int64_t *didx, void *stream) {
  VCMI_TRY(check_xy(g, dX, ldx, T, didx, 1, "vcmi_gmmmap_predict_dev"));
  return gmmmap_predict_device(g, dX, ldx, T, didx, as_stream(stream));
}

extern "C" int vcmi_gmmmap_predict(vcmi_gmmmap *g, const double *X, int64_t ldx, int64_t T, int64_t *idx) {
  VCMI_TRY(check_xy(g, X, ldx, T, idx, 1, "vcmi_gmmmap_predict"));
  if (T == 0) return VCMI_OK;
  return over_frames(g, T, [&](vcmi_gmmmap *r, int64_t lo, int64_t hi) -> int {
    return staged_pipeline(X + lo * ldx, (size_t)r->D * 8, (size_t)ldx * 8, idx + lo, 8, 8, hi - lo, kMinChunkFrames,
                           [&](const void *dIn, void *dOut, int64_t, int64_t n, hipStream_t st) -> int {
                             return gmmmap_predict_device(r, (const double *)dIn, r->D, n, (int64_t *)dOut, st);
                           });
  });
}
