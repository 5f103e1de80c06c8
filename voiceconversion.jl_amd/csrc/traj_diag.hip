// traj_diag.hip -- trajectory conversion with DIAGONAL conditional precisions (vcmi_traj_set_precision, include/vcmi.h).
//
// With the conditional covariance of every mixture taken as diagonal, q_m = 1 ./ diag(Syy_m - A_m Sxy_m) = [p_s ; p_d], the
// blocks of traj.hip's header lose everything that couples: Qsd = Qds = 0, so P[t,t-1] = 0; Qss and Qdd are diagonal, so the D
// static dimensions decouple; only the offsets 0 and +-2 are left, so even and odd frames decouple too.  Per utterance, static
// dimension d and frame parity that is one symmetric tridiagonal system over the frames t = parity, parity + 2, ...:
//   P[t,t]   = p_s(t) + p_d(t-1)/4 + p_d(t+1)/4        r[t] = g_s(t) + g_d(t-1)/2 - g_d(t+1)/2
//   P[t,t-2] = -p_d(t-1)/4                             (terms with a frame outside the utterance dropped, as W drops them)
// with p(t) = q[mhat_t] and g_t = q_mhat (.) (A_mhat x_t + b_mhat) from the g_t kernels of traj.hip, run on the images of
// diag(q_m).  p_s > 0 makes every system strictly diagonally dominant: the Thomas recurrence needs no pivoting and cannot fail.
// Here: the handle's diagonal model (traj_diag_ensure), the solver, the solve entry of the band family (which hands a handle with
// three windows to traj_penta.hip), the setting's two entries.
#include "traj_internal.hpp"
#include "traj_prepare.hpp"
#include "hostpipe.hpp"

namespace vcmi {

// 1/x in FP64: hardware v_rcp_f64 seed + two Newton steps, in the manner of traj_rsqrt -- the one operation of a step that
// sits on the dependent chain.  x is a pivot: positive, finite, far from the ends of the exponent range.
__device__ __forceinline__ double traj_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x);
  y = fma(fma(-x, y, 1.0), y, y);
  y = fma(fma(-x, y, 1.0), y, y);
  return y;
}

// steps whose loads are in flight ahead of the one the chain is at (two rings in the forward sweep: mhat, then what it indexes).
// A forward step issues 6 loads and 2 stores: 48 memory operations in flight at six steps, under the 63 the wave's counter holds
// (eight steps would be 64).
static constexpr int kDiagRing = 6;

// ------------------------------------------------------------------------------------------------
// One wave per (utterance, slab of 32 static dimensions): lanes 0-31 own the even-frame chain of their dimension, lanes 32-63
// the odd-frame chain.  No LDS, no barrier, no cross-lane traffic: a chain's neighbours t +- 1 belong to the other parity and
// are read from gbuf and q[mhat[t +- 1] - 1] in global memory.  Every access of a half-wave is 32 consecutive doubles of a
// (frame, 2D) row (of a (frame, D) row for Y and the workspace).
// Forward, step k at frame t (e_k = P[t,t-2], u_k = e_{k+1} / piv_k, what the back substitution multiplies by):
//   piv_k = P[t,t] - e_k u_{k-1}     z_k = (r_k - e_k z_{k-1}) / piv_k     u_k -> workspace, z_k -> Y
// backward, in place:  y_k = z_k - u_k y_{k+1}.
// Lanes past D in the last slab and steps past the end of a chain (the odd chain of an odd T is one frame shorter; the loop
// runs in whole rings) work on clamped addresses and store nothing: EXEC stays full outside the stores.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
traj_diag_solve_kernel(const TrajUtt *__restrict__ utts, int nslab, int D, const double *__restrict__ q,
                       const int64_t *__restrict__ mhat_all, const double *__restrict__ g_all, double *__restrict__ ws_all) {
  constexpr int R = kDiagRing;
  const int u = (int)(blockIdx.x / (unsigned)nslab), slab = (int)(blockIdx.x % (unsigned)nslab);
  const TrajUtt U = utts[u];
  const int T = U.T;
  if (T == 0) return;
  const int D2 = 2 * D, lane = threadIdx.x, par = lane >> 5;
  const int d0 = slab * 32 + (lane & 31);
  const bool live = d0 < D;
  const int d = live ? d0 : D - 1;
  const int K = (T - par + 1) >> 1, Kmax = (T + 1) >> 1;     // frames of this lane's chain; of the longer of the two
  const int64_t *mh = mhat_all + U.frame0;
  const int *mh32 = reinterpret_cast<const int *>(mh);
  const double *g = g_all + U.frame0 * D2;
  double *cw = ws_all + U.frame0 * D;
  gdouble *Y = (gdouble *)U.Y;
  const int Tl = T - 1;

  // what step k reads that does not depend on the chain: the mixtures of frames t and t + 1 (clamped to the utterance) ...
  auto load_mix = [&](int k, int &m0, int &m1) {
    const int t = par + 2 * k;
    // 1-based, as stored: the rings hold what was loaded and nothing derived from it.  The LOW word alone (1 <= mhat <= M): of
    // an 8-byte load the unused high register is taken for a temporary at once, and writing it waits for every load in flight
    m0 = mh32[2 * (size_t)(t < Tl ? t : Tl)];
    m1 = mh32[2 * (size_t)(t + 1 < Tl ? t + 1 : Tl)];
  };
  // ... and through them p_s(t), g_s(t), p_d(t+1), g_d(t+1)
  auto load_row = [&](int k, int m0, int m1, double &ps, double &gs, double &pdn, double &gdn) {
    const int t = par + 2 * k;
    const size_t t0 = (size_t)(t < Tl ? t : Tl), t1 = (size_t)(t + 1 < Tl ? t + 1 : Tl);
    ps = q[(size_t)(m0 - 1) * D2 + d];
    gs = g[t0 * D2 + d];
    pdn = q[(size_t)(m1 - 1) * D2 + D + d];
    gdn = g[t1 * D2 + D + d];
  };

  int m0r[R], m1r[R];
  double psr[R], gsr[R], pdr[R], gdr[R];
#pragma unroll
  for (int j = 0; j < R; ++j) load_mix(j, m0r[j], m1r[j]);
  // the neighbour below the first frame of the chain: frame 0 for the odd chain, none for the even one
  double pdp = 0.0, gdp = 0.0;
  {
    const double p0 = q[(size_t)((int)mh[0] - 1) * D2 + D + d], g0 = g[D + d];
    pdp = par ? p0 : 0.0;
    gdp = par ? g0 : 0.0;
  }
#pragma unroll
  for (int j = 0; j < R; ++j) load_row(j, m0r[j], m1r[j], psr[j], gsr[j], pdr[j], gdr[j]);
#pragma unroll
  for (int j = 0; j < R; ++j) load_mix(R + j, m0r[j], m1r[j]);

  double uprev = 0.0, zprev = 0.0;
  for (int kb = 0; kb < Kmax; kb += R) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int k = kb + j, t = par + 2 * k;
      const double ps = psr[j], gs = gsr[j];
      const bool nxt = t + 1 < T;
      const double pdn = nxt ? pdr[j] : 0.0, gdn = nxt ? gdr[j] : 0.0;
      const double e = -0.25 * pdp;
      const double dg = ps + 0.25 * pdp + 0.25 * pdn;
      const double r = gs + 0.5 * gdp - 0.5 * gdn;
      const double rp = traj_rcp(fma(-e, uprev, dg));
      const double z = fma(-e, zprev, r) * rp;
      uprev = -0.25 * pdn * rp;
      zprev = z;
      pdp = pdn;
      gdp = gdn;
      if (live && k < K) {
        cw[(size_t)t * D + d] = uprev;
        Y[(size_t)t * D + d] = z;
      }
      // the slots of the step just done take the loads of steps k + R and k + 2R -- issued AFTER their last use: a slot
      // whose old and new value are live together costs a register copy at the loop's end, which waits for every load
      load_row(k + R, m0r[j], m1r[j], psr[j], gsr[j], pdr[j], gdr[j]);
      load_mix(k + 2 * R, m0r[j], m1r[j]);
    }
  }

  // back substitution from the last frame of the chain; the ring holds z and u of the R steps below the current one
  const int Kr = (Kmax + R - 1) / R * R;
  auto load_back = [&](int k, double &z, double &uu) {
    int t = par + 2 * (k > 0 ? k : 0);
    t = t < Tl ? t : Tl;
    z = Y[(size_t)t * D + d];
    uu = cw[(size_t)t * D + d];
  };
  double zr[R], ur[R];
#pragma unroll
  for (int j = 0; j < R; ++j) load_back(Kr - 1 - j, zr[j], ur[j]);
  double ynext = 0.0;
  for (int kb = Kr - 1; kb >= 0; kb -= R) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int k = kb - j, t = par + 2 * k;
      const bool on = k < K;                       // (steps past the end of the chain leave y_{k+1} = 0)
      const double y = on ? fma(-ur[j], ynext, zr[j]) : 0.0;
      ynext = y;
      if (live && on) Y[(size_t)t * D + d] = y;
      load_back(k - R, zr[j], ur[j]);
    }
  }
}

int traj_penta_launch(vcmi_traj *t, const TrajSolvePlan &p, const double *q, const int64_t *mh, hipStream_t st);     // traj_penta.hip

int traj_band_solve_launch(vcmi_traj *t, const TrajSolvePlan &p, const double *q, const int64_t *mh, hipStream_t st) {
  if (t->windows == 3) return traj_penta_launch(t, p, q, mh, st);
  const int nslab = (t->D + 31) / 32;
  hipLaunchKernelGGL(traj_diag_solve_kernel, dim3((unsigned)((int64_t)p.n * nslab)), dim3(64), 0, st, p.du, nslab, t->D, q, mh,
                     t->gbuf.p, t->ws.p);
  VCMI_HIP(hipGetLastError());
  return VCMI_OK;
}

int traj_diag_ensure(vcmi_traj *t) {
  if (t->diag_ready) return VCMI_OK;      // (always so for a cross-diagonal handle: vcmi_traj_create_bdiag, g is NULL)
  const vcmi_gmmmap *g = t->g;
  TrajDiagModel dm;     // the host arithmetic: traj_prepare.cpp
  VCMI_TRY(traj_prepare_diag(g->h_A, g->h_Sxy, g->h_Syy, t->D2, t->M, dm));
  const struct {
    DevBuf<double> &dev;
    const std::vector<double> &host;
  } images[] = {{t->dg_q, dm.q}, {t->dg_QT, dm.QT}, {t->dg_Qfrag, dm.Qfrag}};   // (nothing on the device reads the row-major image)
  for (auto &im : images) {
    VCMI_TRY(im.dev.alloc(im.host.size()));
    const hipError_t e = upload_now_hip(im.dev.p, im.host.data(), im.host.size() * 8);
    if (e != hipSuccess) return fail(VCMI_ERR_HIP, "vcmi_traj_set_precision: upload failed: %s", hipGetErrorString(e));
  }
  t->diag_ready = true;
  return VCMI_OK;
}

}  // namespace vcmi

using namespace vcmi;

extern "C" int vcmi_traj_set_precision(vcmi_traj *t, int kind) {
  if (!t) return fail(VCMI_ERR_ARG, "vcmi_traj_set_precision: NULL handle");
  if (kind != VCMI_TRAJ_PRECISION_FULL && kind != VCMI_TRAJ_PRECISION_DIAG)
    return fail(VCMI_ERR_ARG, "vcmi_traj_set_precision: unknown kind %d", kind);
  if (kind == VCMI_TRAJ_PRECISION_FULL && t->b)
    return fail(VCMI_ERR_ARG, "vcmi_traj_set_precision: the converter was made from a cross-diagonal model (vcmi_traj_create_bdiag): "
                              "its conditional precisions are diagonal, there is no full matrix to switch to");
  if (kind == VCMI_TRAJ_PRECISION_DIAG) {
    if (t->em_iters > 0 && !t->b)      // the M-step blends full precision matrices (a cross-diagonal handle is DIAG already)
      return fail(VCMI_ERR_ARG, "vcmi_traj_set_precision: the converter has EM re-estimation switched on (vcmi_traj_set_em)");
    VCMI_TRY(traj_diag_ensure(t));
  }
  t->precision = kind;
  return VCMI_OK;
}
extern "C" int vcmi_traj_get_precision(const vcmi_traj *t) { return t ? t->precision : -1; }
