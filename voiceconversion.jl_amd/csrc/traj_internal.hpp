// traj_internal.hpp -- what crosses traj.hip, traj_solve.hip, the band family (traj_diag.hip, traj_penta.hip, traj_gv_band.hip),
// traj_gv.hip, traj_em.hip, traj_em_bdiag.hip and traj_vc.cpp: the two handles, the per-call descriptors and HOST functions (no
// relocatable device code: a kernel is launched by the file that defines it).
#pragma once
#include "vcmi_common.hpp"
#include "gmmmap_handle.hpp"
#include "gmmmap_bdiag_handle.hpp"

namespace vcmi {
struct EmTimes {           // what vcmi_debug_traj_em_times reports
  double estep_ms = 0, gbar_ms = 0, blend_ms = 0, solve_ms = 0;   // E-step; gbar; flag scan + count read + blend; pad + solve
  int64_t mixed_frames = 0, frames = 0, slices = 0;               // summed over slices and iterations
  size_t table_bytes = 0;                                         // the largest table
};
}  // namespace vcmi

struct vcmi_traj {
  vcmi_gmmmap *g = nullptr;
  // A converter made straight from a cross-diagonal model (vcmi_traj_create_bdiag) has b in place of g: precision is DIAG for
  // good, dg_q holds b's q, the arg-max and g_t of a call are one pass of b's kernel (bdmap_traj_device), and every dense
  // buffer below (AT .. Afrag, Qpad, cm, dg_QT, dg_Qfrag) stays empty.  No replicas: b converts on its own device.
  vcmi_bdmap *b = nullptr;
  int D2 = 0;          // dim(t) = 2D (static + delta), src/trajectory_gmmmap.jl:35; 3D for a handle with three windows
  int windows = 2;     // 3: static + delta + delta-delta (vcmi_traj_create_bdiag_windows; a cross-diagonal handle only): the
                       // pentadiagonal solver of traj_penta.hip in place of traj_diag.hip's
  int D = 0;           // static dimension
  int M = 0;
  int64_t length = 0;  // length(t), src/trajectory_gmmmap.jl:34
  vcmi::DevBuf<double> AT, QT, bvec, Q;   // [M][k][r] transposed A and Q (coalesced gemv), b [M][2D], Q row-major [M][2D][2D]
  vcmi::DevBuf<double> Qfrag, Afrag;      // Q and A in v_mfma_f64_16x16x4 A-operand order [M][row tile][k-step][lane]
  vcmi::DevBuf<int> gperm;                // frames of every utterance grouped by mixture (traj_g_mfma_kernel)
  int NT = 0, KS = 0;                     // row tiles / k-steps of Qfrag
  vcmi::DevBuf<double> gbuf, ws, xbuf, ybuf;
  // Static dimensions without an instantiation of the blocked solver run in the next larger one (Dpad): Qpad is Q with
  // the extra static dimensions decoupled (unit diagonal in Qss, zeros elsewhere), gpad / ypad the padded right-hand
  // sides and solutions of a call
  int Dpad = 0;
  vcmi::DevBuf<double> Qpad, gpad, ypad;
  bool big = false;                       // static D beyond the LDS-window solvers (D >= 47): traj_solve_big_kernel, window in HBM
  vcmi::DevBuf<double> gwin;
  vcmi::DevBuf<unsigned char> uttpad;
  vcmi::DevBuf<int64_t> mhat;
  vcmi::DevBuf<int> status;
  vcmi::DevBuf<unsigned char> uttbuf;
  // converters on the other devices of a device group (vcmi_set_devices), made lazily by the members' worker threads
  std::vector<vcmi_traj *> replicas;
  uint64_t replicas_epoch = 0;
  // EM re-estimation over all mixtures (traj_em.hip): n >= 0 E/M pairs after the arg-max solution
  int em_iters = 0;
  bool em_pd = false;                     // (Q_m + Q_m') / 2 positive definite for every m: c_m exists
  vcmi::DevBuf<double> cm;                // [M] c_m - D log 2 pi
  vcmi::DevBuf<double> em_lp, em_gamma, em_lse, em_table, em_L;   // log pi and gamma (frames, M); lse (frames); [Q_1..Q_M | Qbar of the mixed frames]; L (iteration, utterance)
  vcmi::DevBuf<int> em_pure, em_mix;      // per frame: mixture of a pure frame or -1; the mixed frames, then their count
  vcmi::DevBuf<int64_t> em_mh;            // table index + 1 per frame
  vcmi::DevBuf<int32_t> em_jobs;          // cross-diagonal EM (traj_em_bdiag.hip): the tile jobs of a call, (utterance, first frame)
  int em_run_iters = 0, em_run_n = 0;     // shape of em_L in the last call
  std::vector<double> em_hist;            // L at each E-step of the last call, summed over its utterances
  bool em_time = false;                   // measurement hook (vcmi_debug_traj_em_times): hip events around the steps of an iteration
  vcmi::EmTimes em_times;                 // ... accumulated since the hook last read them
  size_t em_cap_bytes = 0;                // test hook: table cap in place of kTrajEmTableCapBytes (0: the constant)
  // diagonal conditional precisions (vcmi_traj_set_precision, traj_diag.hip): made on the first switch to DIAG, then kept
  int precision = VCMI_TRAJ_PRECISION_FULL;
  bool diag_ready = false;
  vcmi::DevBuf<double> dg_q, dg_QT, dg_Qfrag;   // q [M][2D]; diag(q_m) in the layouts of QT and Qfrag
  ~vcmi_traj() {
    for (vcmi_traj *r : replicas) delete r;
  }
};

// TrajectoryGVGMMMap(tgmm, mu^v, Sigma^vv), src/trajectory_gmmmap.jl:114-130
struct vcmi_trajgv {
  vcmi_traj *t = nullptr;
  vcmi::DevBuf<double> muv, pv;   // (D), (D,D) = inv(Sigma^vv) in the Julia memory image
  std::vector<double> h_muv, h_pv;             // host copies for the device-group replicas
  bool diag = false;              // made by vcmi_trajgv_create_diag / _bdiag: converts only while t's precision is DIAG (traj_gv_band.hip)
  std::vector<vcmi_trajgv *> replicas;
  uint64_t replicas_epoch = 0;
  ~vcmi_trajgv() {
    for (vcmi_trajgv *r : replicas) delete r;
  }
};

namespace vcmi {

struct TrajGV {          // per-call parameters of the GV ascent
  const double *muv, *pv;
  int epochs;
  double alpha;
};

struct TrajUtt {
  const double *X;   // (2D,T) dense
  double *Y;         // (D,T) dense
  int64_t frame0;    // offset of this utterance in the packed per-frame scratch (mhat, g)
  int32_t T;
  int32_t idx;       // position in the caller's batch (the list is sorted by length before the launch)
};

// A pointer read from a descriptor in memory has no known address space: every access through it is a FLAT
// instruction (both wait counters, no saddr form).  The utterance matrices are global memory: say so.
typedef double __attribute__((address_space(1))) gdouble;

// 1/sqrt(x) in FP64: hardware v_rsq_f64 seed + two Newton steps (each roughly doubles the correct bits; the seed
// has >= 26) -- a short dependent chain instead of the IEEE sqrt + divide expansion on the per-column critical path.
__device__ __forceinline__ double traj_rsqrt(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * fma(-0.5 * x * y, y, 1.5);
  y = y * fma(-0.5 * x * y, y, 1.5);
  return y;
}

// ---- traj_solve.hip ----
// What one traj_run decides about its solves, once (traj_solve_plan): the solver, its operands and its workspace.
struct TrajSolvePlan {
  int n = 0, Tmax = 0;                          // utterances of the call and the longest of them
  int64_t nframes = 0;
  int cus = 256, grid = 0;                      // compute units; min(n, cus): workgroups of the generic, big and GV kernels
  bool padded = false;                          // the blocked solver runs in t->Dpad, on Qpad / gpad / ypad
  int Ds = 0;                                   // static dimension of the solver's operands: t->Dpad when padded, else t->D
  int64_t ws_stride = 0, ws_stride_s = 0;       // workspace doubles per workgroup in D (generic, big, GV) / in Ds (blocked)
  const TrajUtt *du = nullptr, *dus = nullptr;  // the sorted descriptors on the device; dus: with Y in ypad when padded
  const double *gs = nullptr;                   // right-hand sides of the blocked solver: gbuf, or gpad when padded
  int occ = 1;                                  // workgroups per CU of the blocked factorisation kernel
  bool blk = false;                             // the blocked solver runs: Ds has an instantiation and kDbgTrajGeneric is off
};
// D >= 47: the window of the solve does not fit LDS (traj_solve_big_kernel)
bool traj_solve_is_big(int D);
// The plan of a call over `utts` (sorted longest first, ALREADY uploaded to t->uttbuf; t->gbuf reserved; traj_run calls it after
// the g_t launch, so this host work overlaps that kernel); with_gv: the workspace
// also holds the GV ascent's V, r and perm (in diagonal mode: its (nframes,D) arrays).  Host work only, nothing goes to a stream: reserves ws (the one reserve of the solve
// path), gpad / ypad / gwin where the solver needs them, and uploads the padded descriptors (synchronous).  A reserve that
// grows a buffer frees the old one, which waits for the device.  A handle in diagonal mode gets n, Tmax, nframes, du, cus, grid and a
// workspace of band_ws_doubles (traj_band_plan.hpp: one (nframes,D) array over two windows, two over three, five with_gv), its
// size in ws_stride: no padded copies, no window, no occupancy query.
int traj_solve_plan(vcmi_traj *t, const std::vector<TrajUtt> &utts, int64_t nframes, int Tmax, bool with_gv, TrajSolvePlan *plan);
// Solve of the (sorted) utterances [b0, b0 + nb) with the precision table Qs (indexed by mh[t] - 1: t->Q / t->Qpad with t->mhat,
// or the EM loop's table; in plan.Ds) and the right-hand sides in t->gbuf: gbuf -> gpad where padded, the solver the plan chose,
// ypad -> the utterances' Y after a padded solve.  Asynchronous on st, in launch order; t->status must have been zeroed on st.
int traj_solve_launch(vcmi_traj *t, const TrajSolvePlan &plan, const double *Qs, const int64_t *mh, int b0, int nb, hipStream_t st);

// ---- the band family: diagonal conditional precisions (traj_diag.hip, traj_penta.hip, traj_gv_band.hip) ----
// The diagonal model of the handle on the current device (traj_prepare_diag + upload), once; VCMI_ERR_NOT_PD from the host
// arithmetic.  Synchronous.
int traj_diag_ensure(vcmi_traj *t);
// Solve of the plan's utterances with diagonal conditional precisions, by t->windows: the tridiagonal solver of traj_diag.hip (2)
// or the pentadiagonal one of traj_penta.hip (3).  Right-hand sides in t->gbuf [frame][windows D] (made with the diagonal images),
// the precision table q [.][windows D] indexed by the low 32 bits of mh[t] - 1 (t->dg_q with t->mhat, or the cross-diagonal EM
// loop's per-frame table with its identity index); workspace t->ws, the solver's (nframes,D) arrays of traj_band_plan.hpp indexed
// by frame0 (a plan made in diagonal mode).  Asynchronous on st; never writes t->status.
int traj_band_solve_launch(vcmi_traj *t, const TrajSolvePlan &plan, const double *q, const int64_t *mh, hipStream_t st);
// The GV ascent behind that solve, by t->windows: traj_gvd_kernel (2) or traj_gvp_kernel (3) of traj_gv_band.hip; how much of the
// working set stays in LDS follows traj_band_plan.hpp from D and plan.Tmax.  Reads t->mhat, t->gbuf, t->dg_q; workspace: the
// (nframes,D) arrays of the ascent in t->ws, behind the tridiagonal solver's array or on the pentadiagonal solver's two (a plan
// made in diagonal mode with_gv).  Asynchronous on st.
int traj_band_gv_launch(vcmi_traj *t, const TrajSolvePlan &plan, const TrajGV &gv, hipStream_t st);
// VCMI_ERR_ARG for a handle with three windows at an entry that has no three-window form (`what` names it in the message)
int traj_two_windows_only(const vcmi_traj *t, const char *who, const char *what);

// ---- traj_gv.hip ----
// The GV ascent on the solved trajectories of the plan's utterances, in place (two-team kernel where the frame permutation of
// the longest fits LDS, else the one-team kernel; traj_gvw_kernel for more than six row tiles, 2D > 96).  Reads t->mhat, t->gbuf,
// t->Qfrag; workspace: t->ws with plan.ws_stride (a plan made with_gv).  Asynchronous on st, behind the solve.
int traj_gv_launch(vcmi_traj *t, const TrajSolvePlan &plan, const TrajGV &gv, hipStream_t st);
// the checks of a call on a TrajectoryGVGMMMap (T may be NULL) and the per-call parameters of its GV ascent; no device work
int trajgv_args(const vcmi_trajgv *h, int64_t n, const int64_t *T, int epochs, TrajGV *gv);

// ---- traj_em.hip ----
// t->em_iters E/M pairs after the arg-max solve of traj_run, on st behind it; every M-step is a traj_solve_launch.  One 4-byte
// read per iteration synchronises st.  utts: the sorted list the plan was made for.
int traj_em_run(vcmi_traj *t, const std::vector<TrajUtt> &utts, const TrajSolvePlan &plan, bool contiguous, const double *dX0,
                hipStream_t st);
// The EM scratch of a call follows the rule of the vc scratch (postf.hpp): released above kVcScratchKeepBytes.  The caller
// has made sure that nothing on the device still uses it.
void traj_em_release(vcmi_traj *t);
// ... on every way out of a conversion entry, an error return between the EM loop and the status read included: waits for the
// device first
struct TrajEmRelease {
  vcmi_traj *t;
  ~TrajEmRelease();
};
// L[U.idx] = sum of lse over the frames of each of the n utterances du, in a fixed order (traj_em_sum_kernel).  Asynchronous on st.
int traj_em_sum_launch(const TrajUtt *du, int n, const double *lse, double *L, hipStream_t st);

// ---- traj_em_bdiag.hip ----
// t->em_iters E/M pairs over a cross-diagonal handle (t->b) after the arg-max solve of traj_run, on st behind it: per iteration
// the fused E-step + M-step sums, traj_em_sum_launch and traj_band_solve_launch on the per-frame table.  Nothing is read back inside
// the loop; the job list is uploaded once (synchronous) before it.  utts: the sorted list the plan was made for.
int traj_em_bdiag_run(vcmi_traj *t, const std::vector<TrajUtt> &utts, const TrajSolvePlan &plan, hipStream_t st);

// ---- traj.hip ----
// fvconvert of the utterances (dense X and Y on the device; the list comes back sorted longest first): arg-max, g_t, solve, the EM
// loop when t->em_iters > 0, the GV ascent when gv.  contiguous: the X matrices lie back to back from dX0.  Asynchronous on st
// except for the EM loop's reads; follow with traj_check_status.
int traj_run(vcmi_traj *t, std::vector<TrajUtt> &utts, int64_t nframes, bool contiguous, const double *dX0, hipStream_t st,
             const TrajGV *gv = nullptr);
// Reads the status word of the solves (VCMI_ERR_NOT_PD) and the EM objective into t->em_hist; synchronises st.
int traj_check_status(vcmi_traj *t, hipStream_t st);
// Host-pointer batch (checks its arguments): on the current device, or split over the device group; blocking.  gvh: the
// handle behind gv, for its replicas on the group's other devices.
int traj_host_batch(vcmi_traj *t, int64_t n, const double *const *X, const int64_t *T, double *const *Y, const TrajGV *gv = nullptr,
                    vcmi_trajgv *gvh = nullptr);

#ifdef TRAJ_BLK_PROF
// the probe build's cycle counters of each file, printed to stderr and zeroed; synchronise st
void traj_solve_prof_dump(hipStream_t st);
void traj_gv_prof_dump(hipStream_t st);
#endif

}  // namespace vcmi
