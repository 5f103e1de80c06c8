/*
 * vcmi.h -- C-ABI of libvcmi.so: the MI355X (gfx950) hot path of r9y9/VoiceConversion.jl.
 *
 * The reference is pure Julia and has no FFI of its own; its boundary is the exported Julia API
 * (src/VoiceConversion.jl:12-38, src/dtw.jl:7).  Each entry point below replaces the body of one of
 * those Julia functions and is what the Julia wrapper (voiceconversion.jl_amd/julia/VoiceConversionMI.jl)
 * binds with `ccall((:sym, "libvcmi"), Cint, ...)`; the same symbols are bound from Python ctypes
 * (voiceconversion.jl_amd/_lib.py).  INTEGRATION.md shows both bindings.
 *
 * Conventions
 *   - every array is the Julia memory image: column-major Float64; a (D,T) feature matrix is T frames
 *     of D contiguous doubles (`ld` = distance in doubles between consecutive frames, >= D);
 *   - indices written to callers are Julia's: Int64, 1-based;
 *   - plain "host" entry points take host pointers, copy to the current HIP device, run, copy back and
 *     return when the result is in the caller's buffer; `_dev` entry points take DEVICE pointers and a
 *     hipStream_t (passed as void*; NULL = default stream) and only enqueue work;
 *   - every function returns a vcmi_status; vcmi_last_error() gives the thread-local message.  No C++
 *     exception or abort crosses this boundary.  The Julia wrapper maps VCMI_ERR_DIM ->
 *     DimensionMismatch (src/gmmmap.jl:102, src/trajectory_gmmmap.jl:68, src/align.jl:11-13),
 *     VCMI_ERR_NOT_PD -> PosDefException (raised by MvNormal in src/gmm.jl:17), others -> ErrorException;
 *   - handles are not re-entrant: one handle must not be used from two threads at once (the reference's
 *     GMMMap carries mutable scratch too, src/gmmmap.jl:59).
 *   - stream semantics of the `_dev` entries.  Calls share device scratch that outlives them, on the handle or per host
 *     thread ("State that outlives a call").  Consecutive calls of one thread on ANY streams, non-blocking ones
 *     included, are ordered by the library without a host synchronisation: a call first makes its stream wait for the last
 *     kernel of the previous call that used the same scratch (vcmi_gmmmap_convert_dev / _predict_dev per handle;
 *     vcmi_estep_diag_dev, vcmi_gmm_em_*_estep_dev, vcmi_sp2mc_dev / vcmi_mc2sp_dev, vcmi_variance_scaling_dev,
 *     vcmi_dtw_fit_batch_dev per thread), or it has finished when it returns because it ends with a status read on its
 *     stream (vcmi_estep_full_dev, vcmi_traj_convert_batch_dev, vcmi_trajgv_convert_batch_dev, vcmi_vc_traj_dev,
 *     vcmi_vc_trajgv_dev), or it touches the caller's buffers only (vcmi_gmmmap_posterior_dev, vcmi_push_delta_dev,
 *     vcmi_push_delta2_dev, vcmi_mc2b_dev).  The exception is vcmi_kmeans: see there.
 *     None of this holds for a stream that is being CAPTURED into a graph: the entries are not supported under stream
 *     capture ("State that outlives a call").
 */
#ifndef VCMI_H
#define VCMI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  VCMI_OK = 0,
  VCMI_ERR_DIM = 1,       /* inconsistent dimensions              -> DimensionMismatch */
  VCMI_ERR_NOT_PD = 2,    /* covariance block not positive definite -> PosDefException */
  VCMI_ERR_HIP = 3,       /* HIP runtime / kernel failure */
  VCMI_ERR_OOM = 4,       /* host or device allocation failed */
  VCMI_ERR_ARG = 5,       /* NULL pointer, negative size, unsupported option */
  VCMI_ERR_NO_DEVICE = 6  /* no gfx950 device visible */
} vcmi_status;

const char *vcmi_last_error(void);
const char *vcmi_version(void);
int vcmi_device_count(int *count);
/* Select the HIP device used by this thread's subsequent calls (one process per GPU: LOCAL_RANK). */
int vcmi_set_device(int device);
/* ONE host process driving several GPUs -- what a Julia host is (the reference is a single process, src/common.jl:7-63,
 * bin/train_gmm.jl:103).  vcmi_set_devices(devs, n) makes a device group: one persistent worker thread per listed
 * device.  From then on the HOST-POINTER entry points shard their work over the group and join before returning:
 *   vcmi_gmmmap_convert / vcmi_vc_frames / _posterior / _predict   contiguous frame blocks, no collective;
 *   vcmi_dtw_fit_batch / vcmi_align_batch                          pairs split by cost S*T, no collective;
 *   vcmi_traj_convert_batch / vcmi_vc_traj / vcmi_trajgv_convert_batch   utterances (chunks) split by length, no collective;
 *   vcmi_estep_diag / vcmi_estep_full                              frame blocks, then ONE ncclAllReduce(sum) of the packed
 *                                                                  statistics over RCCL (librccl is loaded on first use).
 * Converters are re-created on the other devices on first use.  The `_dev` entry points are unaffected (they run on the
 * device that owns their pointers).  n = 0 removes the group.  The list may name a device twice (both workers share it;
 * useful to test the sharding on a 1-GPU box) except for the E-step, whose RCCL communicator needs distinct devices. */
int vcmi_set_devices(const int *devices, int n);
int vcmi_get_devices(int *devices, int capacity, int *n);

/* Caller-pinned arrays.  A Julia process keeps its feature matrices across calls (src/common.jl:7-26: `vc(c, fm)` reads fm
 * and returns `converted`; bin/vc.jl:82 calls it once per file on arrays it owns).  vcmi_host_register(ptr, bytes) page-locks
 * [ptr, ptr + bytes) ONCE (hipHostRegister); from then on every host-pointer entry point whose dense input and / or output
 * lies inside a registered range moves it by DMA straight between that array and HBM -- no staging slot, no host memcpy --
 * (vcmi_gmmmap_convert, vcmi_vc_frames' input, vcmi_gmmmap_posterior / _predict: each side independently; a side that is
 * not registered, or strided, keeps the staged path); the plain uploads / downloads of the other entry points (the frame
 * matrix of vcmi_estep_diag / _full, result buffers) go straight from / to a registered array as well.  Arrays pinned by
 * the caller's own runtime (hipHostMalloc /
 * hipHostRegister) are recognised as well.  Results are identical either way.  vcmi_host_unregister(ptr) takes the pointer
 * that was registered; an array must be unregistered before it is freed.  Ranges must not overlap (VCMI_ERR_ARG).
 * What is locked are the WHOLE PAGES inside the array -- its partial first and last page, which it shares with its neighbours on
 * the heap, travel as ordinary copies (unmapping such a shared page at unregistration broke later transfers of the HIP runtime
 * from pageable memory nearby: DESIGN 4b, round 6) -- and an array with less than 1 MB of whole pages is recorded, not locked:
 * its calls stage as before.
 * vcmi_host_is_registered: *flag = 1 when the whole range lies in an array registered here (locked or recorded) or in memory
 * another runtime pinned. */
int vcmi_host_register(void *ptr, size_t bytes);
int vcmi_host_unregister(void *ptr);
int vcmi_host_is_registered(const void *ptr, size_t bytes, int *flag);

/* ---------------------------------------------------------------------------------------------
 * GMMMap -- src/gmmmap.jl:57-118, posterior helpers src/gmm.jl:24-58
 * ------------------------------------------------------------------------------------------- */
typedef struct vcmi_gmmmap vcmi_gmmmap;

/* GMMMap(weights, mu, Sigma; swap=false), src/gmmmap.jl:62-90: weights (M), mu (Dj,M), Sigma (Dj,Dj,M).
 * Splits the joint GMM (:41-52), forms A_m = Sigma^yx_m inv(Sigma^xx_m) (:33-36) and the Cholesky factor
 * of Hermitian(Sigma^xx_m) (src/gmm.jl:16-17) on the host, and uploads the packed per-mixture blocks. */
int vcmi_gmmmap_create(const double *weights, const double *mu, const double *sigma, int Dj, int M, int swap,
                       vcmi_gmmmap **out);
int vcmi_gmmmap_destroy(vcmi_gmmmap *g);
int vcmi_gmmmap_dim(const vcmi_gmmmap *g);          /* dim(g),         src/gmmmap.jl:94 */
int vcmi_gmmmap_ncomponents(const vcmi_gmmmap *g);  /* ncomponents(g), src/gmmmap.jl:95 */
/* g.params.ΣʸˣΣˣˣ⁻¹ (D,D,M), src/gmmmap.jl:21 */
int vcmi_gmmmap_get_A(const vcmi_gmmmap *g, double *A);

/* fvconvert(g, x) for every column of X (D,T) -> Y (D,T); src/gmmmap.jl:101-118.  One launch replaces the
 * frame loop of src/common.jl:17-19.  T = 1 is the reference's per-frame call. */
int vcmi_gmmmap_convert(vcmi_gmmmap *g, const double *X, int64_t ldx, int64_t T, double *Y, int64_t ldy);
int vcmi_gmmmap_convert_dev(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy,
                            void *stream);
/* vc(c::FrameByFrameConverter, fm), src/common.jl:7-26: fm, out are (D+1,T); row 1 (power) is copied. */
int vcmi_vc_frames(vcmi_gmmmap *g, const double *fm, int64_t T, double *out);
/* ... with the VarianceScaling post-filter (src/gv.jl:10-15) as a fused post step: out[2:end,:] = fvpostf(VarianceScaling(sigma2),
 * vc(g, fm)[2:end,:]); sigma2 (D) host vector, NULL = plain vcmi_vc_frames.  The converted matrix never leaves HBM between the
 * conversion and the filter: one upload, one download.  Runs on the calling thread's device (the filter's
 * statistics are over the whole matrix).  Device scratch: fm and the result, 2 (D+1) T doubles in the per-thread staging matrix
 * the vcmi_vc_traj_static family uses, grow-only and freed on return above 256 MiB (see there).  The threshold counts that
 * family's converter input and result on this thread too: when the sum is above it, the call ends with a device-wide wait
 * (hipDeviceSynchronize) and frees all three, also after a small matrix. */
int vcmi_vc_frames_postf(vcmi_gmmmap *g, const double *fm, int64_t T, const double *sigma2, double *out);
/* vc over a batch of utterances, frame by frame: out[u] (D+1,T[u]) is what vcmi_vc_frames_postf(g, fm[u], T[u], sigma2, out[u])
 * gives -- row 1 passed through bit for bit, the post-filter's mean and variance over utterance u's converted frames only --
 * with ONE upload, ONE conversion over the packed (D+1, sum T) matrix, the per-utterance filter in place and one download (see
 * vcmi_vc_traj_batch for the rule and the kernels).  fm, T, out: host arrays of n entries; sigma2 (D) may be NULL.  n = 0 is a
 * no-op, T[u] = 0 is allowed (fm[u], out[u] are not read).  Refused before anything is uploaded or launched, every out[u]
 * untouched: sigma2 with some T[u] = 1: VCMI_ERR_DIM; n < 0, T[u] < 0 or a NULL matrix with T[u] > 0: VCMI_ERR_ARG.  Runs on the
 * calling thread's device.  Device scratch: 2 (D+1) sum T doubles in the per-thread staging matrix of vcmi_vc_frames_postf,
 * under its 256 MiB release rule, and the work lists (4 n + sum T / 128 words). */
int vcmi_vc_frames_batch(vcmi_gmmmap *g, int64_t n, const double *const *fm, const int64_t *T, const double *sigma2,
                         double *const *out);
/* predict_proba(g.px, X) -> P (M,T), src/gmm.jl:24-41 */
int vcmi_gmmmap_posterior(vcmi_gmmmap *g, const double *X, int64_t ldx, int64_t T, double *P);
int vcmi_gmmmap_posterior_dev(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, double *dP, void *stream);
/* predict(g.px, X) -> idx (T), 1-based, first maximum wins; src/gmm.jl:44-58.  The index is exact on every path: a
 * mixture's evaluation is cut short (or, on inputs of 8192 frames or more of a peaked model, skipped after a four-row
 * screen on grouped frames) only when an upper bound of its log-density lies below a log-density that was evaluated. */
int vcmi_gmmmap_predict(vcmi_gmmmap *g, const double *X, int64_t ldx, int64_t T, int64_t *idx);
int vcmi_gmmmap_predict_dev(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, int64_t *didx, void *stream);
/* Kernel selection: 0 = auto (MFMA tile kernel when dim(g), rounded up to a multiple of 4, is one of 16..80 in steps of
 * 4; other dimensions up to 160: the tiled MFMA log-density kernel, followed for fvconvert by a softmax / regression
 * kernel over the mixtures that matter; else the generic VALU kernel), 1 = force the generic VALU kernel, 2 = force the
 * MFMA tile kernel (VCMI_ERR_ARG if unavailable). */
int vcmi_gmmmap_set_kernel(vcmi_gmmmap *g, int which);
/* Posterior pruning of fvconvert (src/gmmmap.jl:109-117 sums over ALL mixtures; this changes which terms are evaluated,
 * not the result): the regression A_m x + b_m of mixture m is skipped for a tile of 16 consecutive frames when
 * l_m < max_k l_k - nats for every frame of the tile, i.e. when its posterior there is below e^-nats.  Default 46.0
 * (1e-20: below the rounding error of the remaining terms; y changes by < 1e-18 relative).  +infinity (or any value
 * >= 1e300) evaluates every mixture for every frame -- the dense loop the flop count of SURVEY 8(d) assumes.
 * VCMI_ERR_ARG for nats < 40 (would be visible in y at double precision) or NaN. */
int vcmi_gmmmap_set_prune(vcmi_gmmmap *g, double nats);
/* Diagnostic counter of the pruning: *evaluated (may be NULL) receives the number of (16-frame tile, mixture) regressions
 * the MFMA fvconvert kernel has evaluated on this handle's device since the counter was last enabled (the dense count is
 * ceil(T / 16) * M per converted matrix); then enable != 0 (re)starts the counter at zero, enable == 0 switches it off
 * (the default: the kernel then updates nothing).  Synchronises with the device. */
int vcmi_gmmmap_prune_stats(vcmi_gmmmap *g, int enable, int64_t *evaluated);
/* What fvconvert does with this handle, for measurement (bench.py prices the matrix pipe with it):
 *   *mfma_issued (may be NULL)  v_mfma_f64_16x16x4 instructions (2048 flop each) the MFMA fvconvert kernel has issued since
 *                               vcmi_gmmmap_prune_stats last enabled the counters (0 while they are off); synchronises;
 *   *shape (may be NULL)        the loop the library chose for this model: 0 dense (prune = +inf), 1 "broad" (every
 *                               whitening tile, one branch around the regression), 2 "peaked" (a wrong mixture is decided
 *                               out on its last whitening tile), 3 "screened" (calls of 8192 frames or more, D <= 48: the
 *                               frames are grouped, the group's own mixture is evaluated, every other one is ruled out -- four
 *                               at a time -- by a lower bound of its distance from the four largest eigenpairs of inv(Sxx),
 *                               survivors are evaluated in full; smaller calls of such a model run shape 2),
 *                               -1 no MFMA tile kernel for this dimension;
 *   *model_active_frac, *model_undecided_frac (may be NULL)  the model properties behind that choice, estimated once at
 *                               creation on 256 frames drawn from the model itself: the mean fraction of the mixtures within
 *                               e^-46 of the best one, and the fraction that the last 16-row whitening tile's share of |z|^2
 *                               alone does NOT put e^-46 under the best one ("peaked" is chosen below 0.35; "screened" when
 *                               the screen's own rows leave at most 0.05 undecided).  The shape selects code, never a result:
 *                               every shape gives the dense loop's y to rounding. */
int vcmi_gmmmap_convert_plan(vcmi_gmmmap *g, int64_t *mfma_issued, int *shape, double *model_active_frac,
                             double *model_undecided_frac);
/* The group radius of shape 3, for measurement.  For every mixture g the library derives at creation, on the host, a radius R_g
 * such that a frame with |z_g|^2 < R_g has every other mixture more than `prune` nats under mixture g (a lower bound of
 * |z_m|^2 + lambda |z_g|^2 from both covariances, up to 128 mixtures); a workgroup all of whose frames belong to one group and lie
 * inside its radius does not run the screen at all.  It skips a proof, never a term: y is the same bit for bit.
 *   *skipped (may be NULL)    workgroups that skipped the screen since vcmi_gmmmap_prune_stats last enabled the counters
 *                             (0 while they are off); synchronises;
 *   *in_use (may be NULL)     1 when the kernel takes the test for this model: decided once, at creation, when at least 254 of
 *                             the 256 frames drawn from the model itself lie inside the radius of their mixture;
 *   *pass_frac (may be NULL)  that share. */
int vcmi_gmmmap_screen_radius_stats(vcmi_gmmmap *g, int64_t *skipped, int *in_use, double *pass_frac);

/* ---------------------------------------------------------------------------------------------
 * Cross-diagonal GMMMap -- frame-by-frame conversion (src/gmmmap.jl:101-118, src/gmm.jl:24-58) with the model that
 * train_gmm(covariance_type="block_diag") returns: the four blocks of every joint covariance are diagonal (Toda, Black,
 * Tokuda 2007).  What vcmi_gmmmap_create gives on the expanded (Dj,Dj,M) covariances, at about 6 D M vector operations per frame
 * instead of M (3 D^2 + 6 D) flop (csrc/gmmmap_bdiag.hip).
 *
 * A handle converts on the device it was created on; a device group (vcmi_set_devices) does not shard its calls.
 * ------------------------------------------------------------------------------------------- */
typedef struct vcmi_bdmap vcmi_bdmap;

/* weights (M), mu (Dj,M), covars (Dj + D, M) = [variances of the Dj rows | D pair cross-covariances], D = Dj / 2: pair d couples
 * the rows d and d + D.  swap != 0 exchanges the halves (src/gmmmap.jl:74-78).  Dj even, 1 <= D <= 128, 1 <= M <= 256, else
 * VCMI_ERR_DIM.  A pair with vx <= 0, vy <= 0, vx vy - c^2 <= 0 or a NaN: VCMI_ERR_NOT_PD, the message names the first such
 * (pair, mixture) in memory order, 1-based, as vcmi_gmm_em_bdiag_create does.  A mixture with weight <= 0 has posterior 0. */
int vcmi_bdmap_create(const double *weights, const double *mu, const double *covars, int Dj, int M, int swap,
                      vcmi_bdmap **out);
int vcmi_bdmap_destroy(vcmi_bdmap *h);
int vcmi_bdmap_dim(const vcmi_bdmap *h);
int vcmi_bdmap_ncomponents(const vcmi_bdmap *h);
/* the regression slopes a = c / vx (D,M) */
int vcmi_bdmap_get_a(const vcmi_bdmap *h, double *a);
/* fvconvert for every column of X (D,T) -> Y (D,T), leading dimensions ldx, ldy >= D; one launch per device-resident call.
 * A frame's result does not depend on the other frames of the call; identical inputs give identical bits. */
int vcmi_bdmap_convert(vcmi_bdmap *h, const double *X, int64_t ldx, int64_t T, double *Y, int64_t ldy);
int vcmi_bdmap_convert_dev(vcmi_bdmap *h, const double *dX, int64_t ldx, int64_t T, double *dY, int64_t ldy, void *stream);
/* predict_proba -> P (M,T) */
int vcmi_bdmap_posterior(vcmi_bdmap *h, const double *X, int64_t ldx, int64_t T, double *P);
int vcmi_bdmap_posterior_dev(vcmi_bdmap *h, const double *dX, int64_t ldx, int64_t T, double *dP, void *stream);
/* predict -> idx (T), 1-based, first maximum wins */
int vcmi_bdmap_predict(vcmi_bdmap *h, const double *X, int64_t ldx, int64_t T, int64_t *idx);
int vcmi_bdmap_predict_dev(vcmi_bdmap *h, const double *dX, int64_t ldx, int64_t T, int64_t *didx, void *stream);
/* vc(c, fm), src/common.jl:7-26: fm, out (D+1,T), row 1 (power) copied; sigma2 (D, host) != NULL: the VarianceScaling filter on
 * the converted rows before the download, as vcmi_vc_frames_postf (T = 1 then: VCMI_ERR_DIM). */
int vcmi_vc_bdmap(vcmi_bdmap *h, const double *fm, int64_t T, const double *sigma2, double *out);
/* the contract of vcmi_vc_frames_batch: out[u] is what vcmi_vc_bdmap(h, fm[u], T[u], sigma2, out[u]) gives, bit for bit */
int vcmi_vc_bdmap_batch(vcmi_bdmap *h, int64_t n, const double *const *fm, const int64_t *T, const double *sigma2,
                        double *const *out);

/* ---------------------------------------------------------------------------------------------
 * DTW --src/dtw.jl:93-145 (fit! + backward), align -- src/align.jl:8-35
 * ------------------------------------------------------------------------------------------- */
/* fit!(DTW(fstep,bstep), template (D,S), sequence (D,T)) -> path (T).  costtable (S,T+1) f64 and
 * backpointer (S,T+1) Int64 are the fields d.costtable / d.backpointer (src/dtw.jl:15-16); pass NULL
 * for both to skip materialising them ("path-only" mode). */
int vcmi_dtw_fit(const double *tmpl, int64_t S, const double *seq, int64_t T, int D, int fstep, int bstep,
                 int64_t *path, double *costtable, int64_t *backpointer);
/* n independent pairs in one launch (one workgroup per pair).  Host pointers. */
int vcmi_dtw_fit_batch(int64_t n, const double *const *tmpl, const int64_t *S, const double *const *seq,
                       const int64_t *T, int D, int fstep, int bstep, int64_t *const *path);
/* Device-resident batch: `feats` is one device buffer holding every (D,len) matrix; pair p has its template at
 * feats + tmpl_off[p] (S[p] frames) and its sequence at feats + seq_off[p] (T[p] frames); its path goes to
 * paths + path_off[p].  Offsets (in elements) and lengths are HOST arrays of n entries. */
/* Stream semantics: the call only enqueues work on `stream`.  The pair descriptors and the per-thread workspaces are
 * shared between calls: every call first makes `stream` wait for the previous call's last kernel (whatever stream that
 * ran on), and the descriptors are copied asynchronously on `stream` from pinned slots -- consecutive calls on any
 * streams, including non-blocking ones, are ordered correctly without a host synchronisation. */
int vcmi_dtw_fit_batch_dev(int64_t n, const double *feats, const int64_t *tmpl_off, const int64_t *S,
                           const int64_t *seq_off, const int64_t *T, int D, int fstep, int bstep, int64_t *paths,
                           const int64_t *path_off, void *stream);
/* align(src (D,S), tgt (D,T)) -> newtgt (D,S); path (T) optional (NULL).  src/align.jl:8-35 */
int vcmi_align(const double *src, int64_t S, const double *tgt, int64_t T, int D, double *newtgt, int64_t *path);
int vcmi_align_batch(int64_t n, const double *const *src, const int64_t *S, const double *const *tgt,
                     const int64_t *T, int D, double *const *newtgt);

/* ---------------------------------------------------------------------------------------------
 * Diagonal-covariance E-step (call site bin/train_gmm.jl:103; math SURVEY A.6)
 * ------------------------------------------------------------------------------------------- */
/* X (Dj,N); w (M); mu, var (Dj,M) -> S0 (M), S1, S2 (Dj,M), loglik (1). */
int vcmi_estep_diag(const double *X, int64_t N, int Dj, int M, const double *w, const double *mu, const double *var,
                    double *S0, double *S1, double *S2, double *loglik);
/* Device X; parameters are HOST arrays (tiny).  dstats is a DEVICE buffer of vcmi_estep_stats_len(Dj,M)
 * doubles laid out [S0 (M) | S1 (Dj,M) | S2 (Dj,M) | loglik] -- one contiguous buffer so that the
 * multi-GPU path is a single all-reduce(sum).  Every sum has a fixed order and nothing depends on earlier calls: identical inputs
 * give identical bits, run to run, thread to thread.  From 65536 frames on (M <= 128, Dj <= 80) there are two paths: frames that
 * ONE mixture owns (every other responsibility exactly 0 in double precision) can be settled by a certified low-precision screen
 * and summed per mixture in one pass over X, the rest goes through the FP64 kernel (csrc/estep_hard.hpp, estep_path.hpp;
 * statistics within 1e-12 of each other).  VCMI_ESTEP_AUTO (default) decides per call, on the device, from a sample of the call's
 * own frames (16 chunks of 1024: at most a quarter without an owner -> the hard-assignment path); vcmi_estep_set_path pins
 * VCMI_ESTEP_HARD or VCMI_ESTEP_SOFT for the calling thread (training loops that must take the same path on every rank).
 * Under VCMI_ESTEP_AUTO a model of at most 16 mixtures never takes the hard-assignment path: its one-tile kernel is the faster
 * one whatever the data (csrc/estep.hip, estep_mfma_launch).
 * Log-densities of competing mixtures are evaluated term by term, (x - mu)^2 / var, wherever the expanded form's
 * rounding-error bound exceeds 1e-10 (variances near min_covar).
 * Accuracy, per mixture m (each of S0[m], S1[:,m], S2[:,m] relative to that mixture's own largest value -- the M-step divides by
 * S0[m]), on every path, for a frame whose best log-density leads mixture m's by g nats:
 *   variances >= 1e-3: relative 1e-9 for g <= 690; 744 <= g < 746.5: absolute 1e-320 (subnormal responsibilities);
 *   g >= 746.5: the frame adds exactly 0 to mixture m;
 *   tighter variances: relative 1e-9 for g < 36; beyond, the frame's contribution to m within e^-36 of its own weight;
 *   loglik within 1e-9 relative.
 * A model whose operands leave the FP32 range of the screen (var below ~1.5e-39, |mu / var| or a margin of 2^114 and more, a
 * NaN parameter) settles no frame by it: every frame goes through the FP64 kernel. */
enum { VCMI_ESTEP_AUTO = 0, VCMI_ESTEP_HARD = 1, VCMI_ESTEP_SOFT = 2 };
int vcmi_estep_set_path(int path);
int vcmi_estep_get_path(int *path);
int64_t vcmi_estep_stats_len(int Dj, int M);
int vcmi_estep_diag_dev(const double *dX, int64_t N, int Dj, int M, const double *w, const double *mu,
                        const double *var, double *dstats, void *stream);

/* Full-covariance E-step -- what the reference's training actually runs: bin/train_gmm.jl:84-89 builds
 * sklearn.mixture.GMM(covariance_type="full") and :103 calls fit.  w (M); mu (Dj,M); sigma (Dj,Dj,M).
 * Statistics S0 (M), S1 (Dj,M), S2 (Dj,Dj,M) = sum_n gamma_nm x_n x_n', loglik; device layout
 * [S0 | S1 | S2 | loglik] of vcmi_estep_full_stats_len(Dj,M) doubles (one all-reduce).  VCMI_ERR_NOT_PD when a
 * covariance is not positive definite.  Accuracy per mixture as vcmi_estep_diag's for ordinary models (frames whose
 * responsibility in a mixture is exactly 0 are skipped by its statistics). */
int64_t vcmi_estep_full_stats_len(int Dj, int M);
int vcmi_estep_full(const double *X, int64_t N, int Dj, int M, const double *w, const double *mu, const double *sigma,
                    double *S0, double *S1, double *S2, double *loglik);
int vcmi_estep_full_dev(const double *dX, int64_t N, int Dj, int M, const double *w, const double *mu,
                        const double *sigma, double *dstats, void *stream);

/* EM state resident on the device -- the loop inside `gmm[:fit](dataset.X')`, bin/train_gmm.jl:84-103
 * (sklearn.mixture.GMM(covariance_type="full", min_covar)).  Parameters and whitening blocks stay in HBM between
 * iterations; one iteration is
 *   vcmi_gmm_em_estep_dev (local statistics of this GPU's frames, asynchronous on `stream`)
 *   -> the caller sums the statistics buffers of all ranks (one RCCL all-reduce; nothing to do on one GPU)
 *   -> vcmi_gmm_em_mstep (w = S0/sum S0, mu = S1/S0, Sigma = S2/S0 - mu mu' + min_covar I, then the Cholesky
 *      whitening of every mixture on the device; returns the log-likelihood the statistics carry).
 * dstats: caller-owned DEVICE buffer of vcmi_estep_full_stats_len(Dj,M) doubles, layout as vcmi_estep_full_dev.
 * vcmi_gmm_em_mstep synchronises the stream and reports VCMI_ERR_NOT_PD if a covariance (initial or updated) is not
 * positive definite. */
typedef struct vcmi_gmm_em vcmi_gmm_em;
int vcmi_gmm_em_create(int Dj, int M, const double *w, const double *mu, const double *sigma, double min_covar,
                       vcmi_gmm_em **out);
int vcmi_gmm_em_destroy(vcmi_gmm_em *h);
int vcmi_gmm_em_estep_dev(vcmi_gmm_em *h, const double *dX, int64_t N, double *dstats, void *stream);
int vcmi_gmm_em_mstep(vcmi_gmm_em *h, const double *dstats, void *stream, double *loglik);
int vcmi_gmm_em_get(vcmi_gmm_em *h, double *w, double *mu, double *sigma);

/* The same loop for a DIAGONAL model (sklearn.mixture.GMM(covariance_type="diag", min_covar); the usual cheap warm start of
 * the full-covariance fit).  The handle owns the parameters on the device as [w (M) | mu (Dj,M) | var (Dj,M)], 1 <= Dj <= 256;
 * one iteration is
 *   vcmi_gmm_em_diag_estep_dev (vcmi_estep_diag_dev's statistics under the handle's parameters, asynchronous on `stream`;
 *      N == 0 gives zeroed statistics)
 *   -> the caller sums the statistics buffers of all ranks (one all-reduce of vcmi_estep_stats_len(Dj,M) doubles)
 *   -> vcmi_gmm_em_diag_mstep (eps = 2^-52:  w = S0 / (sum S0 + 10 eps) + eps,  inv = 1 / (S0 + 10 eps),  mu = S1 inv,
 *      var = S2 inv - 2 mu S1 inv + mu mu + min_covar; the sum over M in a fixed order, no floating-point atomics: the same
 *      statistics give the same bits).  It synchronises the stream and returns the log-likelihood the statistics carry.
 * For M <= 128 and an even Dj <= 160 the E-step's preparation kernels read the handle's block: no parameter crosses the
 * host, the call waits for nothing, and its statistics are bit-identical to vcmi_estep_diag_dev called with the values
 * vcmi_gmm_em_diag_get returns (the same paths: vcmi_estep_set_path applies).  Odd Dj, M > 128 and Dj > 160 have no such
 * route -- their host code pads, regroups or transposes the parameters: the handle copies its block to the host, with ONE
 * stream synchronisation per E-step, and calls the host-parameter path (same bits again).
 * VCMI_ERR_NOT_PD: a variance that is not > 0 (a NaN included) -- from create for the initial ones, from mstep for updated
 * ones (the message names the first (d, m) in memory order).  After a failed mstep the handle keeps the parameters the
 * statistics were computed under (vcmi_gmm_em_diag_get shows them), every later mstep fails the same way and
 * vcmi_gmm_em_diag_estep_dev returns VCMI_ERR_NOT_PD without launching. */
typedef struct vcmi_gmm_em_diag vcmi_gmm_em_diag;
int vcmi_gmm_em_diag_create(int Dj, int M, const double *w, const double *mu, const double *var, double min_covar,
                            vcmi_gmm_em_diag **out);
int vcmi_gmm_em_diag_destroy(vcmi_gmm_em_diag *h);
int vcmi_gmm_em_diag_estep_dev(vcmi_gmm_em_diag *h, const double *dX, int64_t N, double *dstats, void *stream);
int vcmi_gmm_em_diag_mstep(vcmi_gmm_em_diag *h, const double *dstats, void *stream, double *loglik);
int vcmi_gmm_em_diag_get(vcmi_gmm_em_diag *h, double *w, double *mu, double *var);

/* CROSS-DIAGONAL ("block_diag") joint model -- Toda, Black and Tokuda (2007): each of the four blocks Sigma^xx, Sigma^xy,
 * Sigma^yx, Sigma^yy is diagonal.  Dj is even, D = Dj / 2; pair d is the joint rows (d, d + D), a 2 x 2 block per pair.
 * covars (Dj + D, M), column-major: rows [0, Dj) the variances (as the diagonal model's var), rows [Dj, Dj + D) the
 * cross-covariances c_dm = cov(z_d, z_{d+D}).  With det = vx vy - c^2, dx = z_d - mu_d, dy = z_{d+D} - mu_{d+D}:
 *   l_nm = log w_m - (Dj log 2 pi + sum_d log det_dm + sum_d (vy dx^2 - 2 c dx dy + vx dy^2) / det_dm) / 2,
 * evaluated in the centred, factorised form dx^2 / vx + (dy - (c / vx) dx)^2 vx / det (no cancellation to repair, also at
 * pair correlations close to +-1).  Statistics: one DEVICE buffer [S0 (M) | S1 (Dj,M) | S2 (Dj,M) | Sxy (D,M) | loglik] of
 * vcmi_estep_bdiag_stats_len(Dj,M) = M (1 + 2 Dj + D) + 1 doubles, each (.,M) part mixture by mixture;
 * Sxy_dm = sum_n gamma_nm z_d z_{d+D}, the rest as vcmi_estep_diag_dev -- one contiguous buffer, one all-reduce(sum).
 * Every even Dj in [2, 256] and every M in [1, 256]; anything else: VCMI_ERR_DIM (the message names the limit).  N == 0 gives
 * zeroed statistics.  A pair is valid when vx > 0, vy > 0 and vx vy - c^2 > 0 (a NaN fails): otherwise VCMI_ERR_NOT_PD, the
 * message names the first (d, m) in memory order, d the pair index.  Every sum has a fixed order and nothing depends on
 * earlier calls: identical inputs give identical bits.
 * Accuracy, per mixture m: each of S0[m], S1[:,m], S2[:,m], Sxy[:,m] within 1e-9 of the exact statistics, relative to that
 * mixture's own largest value; loglik within 1e-9 relative -- variances at min_covar and pair correlations close to +-1
 * included. */
int64_t vcmi_estep_bdiag_stats_len(int Dj, int M);
int vcmi_estep_bdiag_dev(const double *dX, int64_t N, int Dj, int M, const double *w, const double *mu,
                         const double *covars, double *dstats, void *stream);

/* The EM loop for the cross-diagonal model.  The handle owns [w (M) | mu (Dj,M) | covars (Dj + D, M)] on the device; one
 * iteration is
 *   vcmi_gmm_em_bdiag_estep_dev (vcmi_estep_bdiag_dev's statistics under the handle's parameters, asynchronous on `stream`:
 *      no parameter crosses the host, the call waits for nothing; bit-identical to vcmi_estep_bdiag_dev called with the
 *      values vcmi_gmm_em_bdiag_get returns; N == 0 gives zeroed statistics)
 *   -> the caller sums the statistics buffers of all ranks (one all-reduce of vcmi_estep_bdiag_stats_len(Dj,M) doubles)
 *   -> vcmi_gmm_em_bdiag_mstep (eps = 2^-52:  w = S0 / (sum S0 + 10 eps) + eps,  inv = 1 / (S0 + 10 eps),  mu = S1 inv,
 *      var = S2 inv - 2 mu S1 inv + mu mu + min_covar,  c = Sxy inv - mu_d mu_{d+D} (min_covar on variances only); the sum
 *      over M in a fixed order, no floating-point atomics: the same statistics give the same bits).  It synchronises the
 *      stream and returns the log-likelihood the statistics carry.
 * VCMI_ERR_NOT_PD: a pair that is not valid -- from create for the initial parameters, from mstep for updated ones.  After a
 * failed mstep the handle keeps the parameters the statistics were computed under (vcmi_gmm_em_bdiag_get shows them), every
 * later mstep fails the same way and vcmi_gmm_em_bdiag_estep_dev returns VCMI_ERR_NOT_PD without launching. */
typedef struct vcmi_gmm_em_bdiag vcmi_gmm_em_bdiag;
int vcmi_gmm_em_bdiag_create(int Dj, int M, const double *w, const double *mu, const double *covars, double min_covar,
                             vcmi_gmm_em_bdiag **out);
int vcmi_gmm_em_bdiag_destroy(vcmi_gmm_em_bdiag *h);
int vcmi_gmm_em_bdiag_estep_dev(vcmi_gmm_em_bdiag *h, const double *dX, int64_t N, double *dstats, void *stream);
int vcmi_gmm_em_bdiag_mstep(vcmi_gmm_em_bdiag *h, const double *dstats, void *stream, double *loglik);
int vcmi_gmm_em_bdiag_get(vcmi_gmm_em_bdiag *h, double *w, double *mu, double *covars);

/* k-means -- sklearn 0.17 cluster.KMeans, what GMM(init_params="wmc") runs over all of X before the first E-step
 * (bin/train_gmm.jl:84-89).  Centers (Dj,M) column-major, 1 <= Dj <= 256, 1 <= M <= 1024; every distance is the direct
 * difference sum_d (x_d - c_d)^2 (sequential in d, FP64, no contraction); exact ties go to the smaller center index.
 * dX is a dense (Dj,N) DEVICE block (leading dimension Dj).  The handle keeps mind2 (N doubles) and labels (N ints) of
 * the last assignment or seeding pass, so the far / seed calls that follow must pass the same block.
 * Footprint: 3 Dj M + 70 ceil(M/16) ceil(Dj/4) doubles, 12 bytes per frame, statistics partials of at most 128 MB.
 * Summation is deterministic: fixed-order partials, no floating-point atomics.
 *
 * Lloyd iteration (per rank; what crosses ranks is marked):
 *   vcmi_kmeans_assign_dev   local statistics [count (M) | sum x (Dj,M) | inertia] of vcmi_kmeans_stats_len doubles,
 *                            asynchronous; dlabels (N int32, may be NULL) receives the labels.  -> ALL-REDUCE (sum)
 *   vcmi_kmeans_update       centers = sum x / count; returns the summed inertia and the number of empty clusters
 *                            (one synchronising read).  With no empty cluster it also returns the summed squared shift.
 *   (n_empty > 0) vcmi_kmeans_far_dev  this rank's top-n_empty records [mind2, global frame index, x (Dj)] by mind2
 *                            (ties: smaller index; `offset` = global index of the rank's first frame) -> ALL-GATHER
 *                 vcmi_kmeans_relocate  the e-th empty cluster takes the e-th best of the ncand gathered records; shift
 *   The handle tracks the centers of the lowest inertia (as sklearn's best_centers); vcmi_kmeans_restore_best makes them
 *   current for the final relabelling pass.
 * Greedy k-means++ (sklearn _k_init): the host draws every random number.
 *   vcmi_kmeans_seed_commit  center c <- dcenter (Dj, device); mind2 = min(mind2, |x - c|^2) (c == 0: reset);
 *                            *potential = local sum of mind2                                   -> ALL-GATHER (1 double)
 *   vcmi_kmeans_seed_pick    idx[l] = first local frame whose inclusive prefix of mind2 reaches targets[l] (host values
 *                            u_l * potential minus the potential of the ranks before); N - 1 past the end.  The rank that
 *                            owns a pick sends that frame (Dj doubles) to the others.
 *   vcmi_kmeans_seed_trials  local potential sum min(mind2, |x - cand_l|^2) of L <= 16 device candidates cand (Dj,L) in one
 *                            pass                                                             -> ALL-REDUCE (L doubles)
 * VCMI_ERR_ARG for non-finite frames or centers (reported by update / seed_commit), VCMI_ERR_DIM for bad shapes.  The update
 * that reports a non-finite value has already written the centers from those statistics: call vcmi_kmeans_set before the
 * handle is used again.
 * Streams: labels, mind2 and the statistics partials live on the handle and carry NO stream order of their own.  A Lloyd
 * iteration is a chain on one stream that ends in a synchronising read, so none is needed there; two asynchronous calls of
 * ONE handle on different streams (vcmi_kmeans_assign_dev, _far_dev, _mind2_dev) must be ordered by the caller (an event,
 * or the same stream). */
typedef struct vcmi_kmeans vcmi_kmeans;
int64_t vcmi_kmeans_stats_len(int Dj, int M);
int vcmi_kmeans_create(int Dj, int M, const double *centers0, vcmi_kmeans **out);
int vcmi_kmeans_destroy(vcmi_kmeans *h);
int vcmi_kmeans_set(vcmi_kmeans *h, const double *centers);
int vcmi_kmeans_get(vcmi_kmeans *h, double *centers);
int vcmi_kmeans_restore_best(vcmi_kmeans *h);
int vcmi_kmeans_assign_dev(vcmi_kmeans *h, const double *dX, int64_t N, double *dstats, int *dlabels, void *stream);
int vcmi_kmeans_update(vcmi_kmeans *h, const double *dstats, void *stream, double *shift, double *inertia, int *n_empty);
int vcmi_kmeans_far_dev(vcmi_kmeans *h, const double *dX, int64_t N, int E, int64_t offset, double *drec, void *stream);
int vcmi_kmeans_relocate(vcmi_kmeans *h, const double *dstats, const double *dcand, int64_t ncand, void *stream,
                         double *shift);
int vcmi_kmeans_seed_commit(vcmi_kmeans *h, const double *dX, int64_t N, int c, const double *dcenter, void *stream,
                            double *potential);
int vcmi_kmeans_seed_pick(vcmi_kmeans *h, int L, const double *targets, void *stream, int64_t *idx);
int vcmi_kmeans_seed_trials(vcmi_kmeans *h, const double *dX, int64_t N, const double *dcand, int L, void *stream,
                            double *potentials);
/* copy of the handle's mind2 (direct-difference squared distance to the nearest center, N doubles) of the last assignment
 * or seeding pass over a block of N frames, into the device buffer dmind2; asynchronous on `stream` */
int vcmi_kmeans_mind2_dev(vcmi_kmeans *h, int64_t N, double *dmind2, void *stream);

/* ---------------------------------------------------------------------------------------------
 * TrajectoryGMMMap -- src/trajectory_gmmmap.jl:3-110, vc src/common.jl:31-63, push_delta src/datasets.jl:6-13
 * ------------------------------------------------------------------------------------------- */
typedef struct vcmi_traj vcmi_traj;
/* TrajectoryGMMMap(g, T): g's dim is 2D (static+delta); precomputes Dy_m = inv(Sigma^yy_m - A_m Sigma^xy_m)
 * (:24-28).  T only sets length(t) (:34); W is a stencil and is never materialised.  g must outlive t. */
int vcmi_traj_create(vcmi_gmmmap *g, int64_t T, vcmi_traj **out);
/* TrajectoryGMMMap straight from a cross-diagonal model over static+delta features (dim(b) = 2D, the joint model has
 * Dj = 4D and joint row k is coupled with row k + 2D only).  The conditional covariance of such a model is diagonal exactly:
 * q_km = 1 / (vy_km - a_km c_km), a = c / vx, so the result is an ordinary vcmi_traj whose precision is VCMI_TRAJ_PRECISION_DIAG
 * for good -- every entry that takes a vcmi_traj* (vcmi_traj_convert[_batch[_dev]], the vcmi_vc_traj family,
 * vcmi_vc_traj_batch[_dev]) converts with it through the tridiagonal solver.  The dense model is never formed, on the host or
 * on the device: the handle holds q (2D M doubles) and the per-call scratch (mhat, g, workspace, descriptors); the arg-max
 * and g_t = q_mhat (.) (mu_y + a (x - mu_x)) of a call are one pass of b's kernel (csrc/gmmmap_bdiag.hip, mode 3), which reads
 * b's log-density table and a [M][2D][mu_x, a, mu_y, q] table that vcmi_bdmap_create uploads.  mhat is the first maximum of
 * the centred log-density of vcmi_bdmap_predict.  Equal to vcmi_traj_create over the expanded model with
 * vcmi_traj_set_precision(DIAG) to rounding.  b must outlive t.
 * VCMI_ERR_DIM: dim(b) odd.  VCMI_ERR_NOT_PD: a conditional variance that is zero, negative or not finite in FP64 (a valid pair
 * with |c| within rounding of sqrt(vx vy)); the message names the pair.  The handle follows vcmi_bdmap's device rule: it
 * converts on the device b was created on, a device group does not shard its calls, a call from another device is
 * VCMI_ERR_ARG.  VCMI_ERR_ARG, the handle usable afterwards: vcmi_traj_set_precision(t, FULL), vcmi_traj_set_em(t, n > 0),
 * vcmi_traj_cond_loglik[_dev], and every convert entry of a vcmi_trajgv of vcmi_trajgv_create over t (the GV ascent over such a
 * converter: vcmi_trajgv_create_diag). */
int vcmi_traj_create_bdiag(vcmi_bdmap *b, int64_t T, vcmi_traj **out);
/* ... with the window count of the features.  windows = 2: vcmi_traj_create_bdiag exactly.  windows = 3: b is a model over
 * static + delta + delta-delta features, rows [static (D); delta (D); delta-delta (D)], dim(b) = 3D (the joint model has Dj = 6D,
 * joint row k is coupled with row k + 3D only; vcmi_gmm_em_bdiag_* trains it as it is).  W then has three rows per frame and
 * static dimension: the static row, the delta row (-1/2 at t-1, +1/2 at t+1) and the delta-delta row (1 at t-1, -2 at t, 1 at
 * t+1), entries outside the utterance dropped, the -2 always there -- the rows vcmi_push_delta2 makes of a static track.  The
 * normal equations are one symmetric positive definite PENTADIAGONAL system per static dimension over all frames (the frame
 * parities no longer decouple, and the system is not diagonally dominant), solved by L D L' without pivoting in
 * traj_penta_solve_kernel (csrc/traj_penta.hip; statement: csrc/traj_penta_step.hpp): O(T D) work, two D T workspace arrays, no
 * LDS.  The arg-max + g_t pass is vcmi_traj_create_bdiag's, over 3D rows (dim(b) <= 128 as for vcmi_bdmap).  dim(t) = 3D.
 * VCMI_ERR_DIM: windows = 3 with dim(b) % 3 != 0 (the message names static + delta + delta-delta); any other window count:
 * VCMI_ERR_ARG.  VCMI_ERR_NOT_PD and the device rule: vcmi_traj_create_bdiag's.
 * A handle with three windows converts through vcmi_traj_convert, _batch and _batch_dev (X (3D,T)), vcmi_vc_traj,
 * vcmi_vc_traj_postf and vcmi_vc_traj_dev with is_static = 0 (fm (3D+1,T), chunks of length(t), the power row passed through bit
 * for bit).  Follow-ups, not provided yet -- VCMI_ERR_ARG with a message that says three windows, before any launch, the handle
 * usable afterwards: vcmi_vc_traj_static and is_static = 1 of vcmi_vc_traj_dev; the vcmi_vc_traj_batch family;
 * vcmi_traj_set_em_bdiag(t, n > 0); vcmi_traj_cond_loglik_bdiag[_dev]; vcmi_trajgv_create_diag over such a handle (refused when
 * the GV handle is made; the GV ascent over three windows: vcmi_trajgv_create_bdiag).  What vcmi_traj_create_bdiag refuses, a handle with three windows refuses too. */
int vcmi_traj_create_bdiag_windows(vcmi_bdmap *b, int64_t T, int windows, vcmi_traj **out);
/* 2, or 3 for a handle of vcmi_traj_create_bdiag_windows(b, T, 3); -1 for NULL */
int vcmi_traj_get_windows(const vcmi_traj *t);
int vcmi_traj_destroy(vcmi_traj *t);
/* length(t).  As in the reference, fvconvert rebuilds W when the sequence length differs (src/trajectory_gmmmap.jl:70-72),
 * so after vcmi_traj_convert(t, X, T, Y) the length is T, and after vcmi_vc_traj it is the length of the last chunk --
 * which is the chunk length the NEXT vc call uses (src/common.jl:41).  The batch entry points leave it unchanged. */
int64_t vcmi_traj_length(const vcmi_traj *t);
/* fvconvert(t, X (2D,T)) -> Y (D,T); src/trajectory_gmmmap.jl:65-110 */
int vcmi_traj_convert(vcmi_traj *t, const double *X, int64_t T, double *Y);
/* n utterances, one launch; host pointers */
int vcmi_traj_convert_batch(vcmi_traj *t, int64_t n, const double *const *X, const int64_t *T, double *const *Y);
/* device-resident batch: utterance u has X at dX + x_off[u] ((2D,T[u])) and Y at dY + y_off[u] ((D,T[u])) */
int vcmi_traj_convert_batch_dev(vcmi_traj *t, int64_t n, const double *dX, const int64_t *x_off, const int64_t *T,
                                double *dY, const int64_t *y_off, void *stream);
/* Toda'07 eqs. 30-36 instead of the suboptimum sequence of src/trajectory_gmmmap.jl:81-82: n >= 0 EM iterations after
 * the argmax solution.  0 (default) = the reference's conversion, unchanged.  E-step: gamma_{m,t} = P(m | X_t, (W y)_t) at the
 * current y, every mixture (none is pruned); M-step: the same banded solve with Qbar_t = sum_m gamma Q_m and
 * gbar_t = sum_m gamma Q_m E_{m,t} (statement: csrc/traj_em.hip).  The setting belongs to the handle: vcmi_traj_convert,
 * _batch, _batch_dev and the vcmi_vc_traj family (per chunk) honour it, also on the replicas of a device group.
 * iters < 0: VCMI_ERR_ARG; iters > 0 on a model with some (Q_m + Q_m')/2 not positive definite (no log-determinant):
 * VCMI_ERR_NOT_PD -- with 0 such a model converts as before.  A vcmi_trajgv over a handle with iters > 0 returns VCMI_ERR_ARG
 * from every convert entry before anything runs (the GV ascent reads one mixture per frame): EM with GV is not provided, with
 * either kind of GV handle.
 * Device scratch while EM runs, on the handle: log pi and gamma, M T doubles each; lse, flags and indices, ~4 T words; and the
 * precision table (M + n_mixed) (2Ds)^2 doubles, Ds the dimension the solver runs in (D, or the padded one), n_mixed the frames
 * of a slice with 1 - max_m gamma >= 2^-53.  A batch is processed in slices of whole utterances so that the table stays under
 * 16 GiB (kTrajEmTableCapBytes, csrc/postf.hpp): the batch starts as one slice and is cut only where the mixed-frame count of
 * an iteration would take the table past the cap (one utterance is never cut).  That count is read back once per slice and
 * iteration -- the loop's only host synchronisation.  The buffers are released on every return of a conversion entry, an
 * error return included, when together they exceed 256 MiB (kVcScratchKeepBytes).  Every feature dimension the converter
 * accepts converts with EM (2D <= 96 on MFMA tiles, above that one workgroup per frame). */
int vcmi_traj_set_em(vcmi_traj *t, int iters);
int vcmi_traj_get_em(const vcmi_traj *t);
/* The conditional precisions of the conversion.  FULL (default): Dy_m = inv(Sigma^yy_m - A_m Sigma^xy_m), the reference's
 * conversion, launch for launch as before.  DIAG: the conditional covariance of every mixture taken as diagonal, as MLPG is
 * commonly run: q_m = 1 ./ diag(Sigma^yy_m - A_m Sigma^xy_m) (the reciprocals of the conditional variances, not the diagonal of
 * Dy_m).  The normal equations then fall apart into 2 D symmetric tridiagonal systems per utterance -- one per static dimension
 * and frame parity, strictly diagonally dominant -- which traj_diag_solve_kernel (csrc/traj_diag.hip) solves with the Thomas
 * recurrence: O(T D) work instead of O(T D^3), one D T workspace, no LDS, the same cost per dimension for every D.
 * The setting belongs to the handle, like vcmi_traj_set_em: vcmi_traj_convert, _batch, _batch_dev, the vcmi_vc_traj family (per
 * chunk) and vcmi_vc_traj_batch[_dev] honour it, also on the replicas of a device group.  The diagonal model (q and the
 * images of diag(q_m) the g_t kernels read: (M (2D)^2 + M 16 NT 4 KS + 2 D M) doubles) is built and uploaded on the first
 * switch to DIAG, on the calling thread's device, and kept.
 * VCMI_ERR_NOT_PD: a conditional variance that is zero, negative or not finite.  VCMI_ERR_ARG, the setting unchanged: an unknown
 * kind; DIAG on a handle with EM iterations > 0, and vcmi_traj_set_em(t, n > 0) on a DIAG handle.  Every convert entry of a
 * vcmi_trajgv made by vcmi_trajgv_create returns VCMI_ERR_ARG before anything runs while its converter is DIAG; one made by
 * vcmi_trajgv_create_diag converts exactly then (below).  vcmi_traj_cond_loglik[_dev] ignores the setting:
 * it always evaluates the full-covariance model. */
#define VCMI_TRAJ_PRECISION_FULL 0
#define VCMI_TRAJ_PRECISION_DIAG 1
int vcmi_traj_set_precision(vcmi_traj *t, int kind);
int vcmi_traj_get_precision(const vcmi_traj *t);
/* L(y) = log P(W y | X) of the statement above for one utterance: X (2D,T), Y (D,T).  VCMI_ERR_NOT_PD where the objective is
 * undefined (see above).  The _dev entry takes dense device matrices and writes *dL on `stream`; it first waits for `stream`
 * and uploads a 32-byte descriptor synchronously (the descriptor buffer is shared with the conversion entries), the kernels
 * then run asynchronously.  Scratch: log pi and gamma, 2 M T doubles on the handle; the host entry releases it above 256 MiB,
 * the _dev entry, which returns before its kernels end, leaves it to the next conversion or host call. */
int vcmi_traj_cond_loglik(vcmi_traj *t, const double *X, const double *Y, int64_t T, double *L);
int vcmi_traj_cond_loglik_dev(vcmi_traj *t, const double *dX, const double *dY, int64_t T, double *dL, void *stream);
/* objective at each E-step of the handle's last conversion call, summed over its utterances: min(cap, iters) values
 * (entry k = L(y^k), k = 0 .. iters-1; entries beyond the iterations of that call are NaN) */
int vcmi_traj_em_history(const vcmi_traj *t, double *L, int cap);
/* The same re-estimation over a handle of vcmi_traj_create_bdiag (any other handle: VCMI_ERR_ARG; iters < 0: VCMI_ERR_ARG), in
 * closed form on the vector pipe: the conditional covariance of a cross-diagonal model is diagonal exactly, so Q_m = diag(q_m),
 * the quadratic form is sum_k q_km e_k^2, the blended precision of a frame is a vector of 2D doubles and the M-step is the
 * tridiagonal solve of vcmi_traj_set_precision(DIAG) over a per-frame table (statement: csrc/traj_em_bdiag.hip).  One fused
 * kernel per iteration does the E-step and both M-step sums, then the per-utterance objective and the solve; nothing per
 * (frame, mixture) goes to HBM and nothing is read back inside the loop.  vcmi_traj_get_em and vcmi_traj_em_history report the
 * setting and the objective; vcmi_traj_convert, _batch, _batch_dev, the vcmi_vc_traj family and vcmi_vc_traj_batch[_dev] honour
 * it; with 0 the handle issues the launches of vcmi_traj_create_bdiag alone.  vcmi_traj_set_em(t, n > 0) keeps refusing such
 * a handle.  Every convert entry of a vcmi_trajgv of vcmi_trajgv_create_diag over t returns VCMI_ERR_ARG while iters > 0 (GV over
 * re-estimated trajectories is not provided) and converts again after vcmi_traj_set_em_bdiag(t, 0).
 * Device scratch while EM runs, on the handle, for the N frames of a call: qbar, 2D N doubles; lse and the identity index the
 * solver reads, N words each (N > 2^31 - 2: VCMI_ERR_DIM before any launch); the tile job list, 8 bytes per 64 (or 32) frames;
 * released as vcmi_traj_set_em's. */
int vcmi_traj_set_em_bdiag(vcmi_traj *t, int iters);
/* L(y) = log P(W y | X) for a handle of vcmi_traj_create_bdiag: vcmi_traj_cond_loglik[_dev]'s arguments and rules, evaluated by
 * the fused kernel's L-only mode. */
int vcmi_traj_cond_loglik_bdiag(vcmi_traj *t, const double *X, const double *Y, int64_t T, double *L);
int vcmi_traj_cond_loglik_bdiag_dev(vcmi_traj *t, const double *dX, const double *dY, int64_t T, double *dL, void *stream);
/* vc(c::TrajectoryConverter, fm (2D+1,T)) -> out (D+1,T) in chunks of length(t) frames; src/common.jl:31-63 */
int vcmi_vc_traj(vcmi_traj *t, const double *fm, int64_t T, double *out);
/* push_delta(src (D,T)) -> out (2D,T); src/datasets.jl:6-13.  Host matrices, host arithmetic (O(DT), no device needed). */
int vcmi_push_delta(const double *src, int D, int64_t T, double *out);
/* ... and on DEVICE-RESIDENT matrices with leading dimensions (lds >= D, ldo >= 2D), asynchronous on `stream`: the input of
 * the trajectory conversion is built where the features already are (bin/vc.jl:75-78 builds it in front of vc). */
int vcmi_push_delta_dev(const double *dsrc, int64_t lds, int D, int64_t T, double *dout, int64_t ldo, void *stream);
/* push_delta with a delta-delta block: src (D,T) -> out (3D,T).  Rows 1 .. 2D are vcmi_push_delta's bit for bit (the first and
 * the last frame keep the reference's static copy in the delta rows).  Rows 2D+1 .. 3D are x_{t-1} - 2 x_t + x_{t+1} with a
 * neighbour outside the matrix dropped: a_1 = -2 x_1 + x_2, a_T = x_{T-1} - 2 x_T, T = 1 gives -2 x_1 -- the convention of W
 * (vcmi_traj_create_bdiag_windows), so the delta-delta rows of a training matrix are exactly the delta-delta rows of W x.  Host
 * arithmetic; the _dev form (lds >= D, ldo >= 3D) is one streaming kernel on `stream`, touches the caller's buffers only, and
 * gives the host routine's values bit for bit. */
int vcmi_push_delta2(const double *src, int D, int64_t T, double *out);
int vcmi_push_delta2_dev(const double *dsrc, int64_t lds, int D, int64_t T, double *dout, int64_t ldo, void *stream);
/* vc(c::TrajectoryConverter, fm) with the VarianceScaling post-filter (src/gv.jl:10-15) applied to the converted rows
 * 2..D+1 BEFORE the download: out[2:end,:] = fvpostf(VarianceScaling(sigma2), vc(t, fm)[2:end,:]); sigma2 (D) host vector,
 * NULL = plain vcmi_vc_traj.  One upload, one download; everything in between stays in HBM.  With sigma2 this is
 * vcmi_vc_traj_static's routine on the (2D+1,T) matrix: its rules (T = 0, T < 2, length(t), device) and its scratch, (6D+2) T
 * doubles here -- converter input, result, and the staging matrix with the (D+1,T) result behind fm -- freed on return above
 * 256 MiB. */
int vcmi_vc_traj_postf(vcmi_traj *t, const double *fm, int64_t T, const double *sigma2, double *out);
/* bin/vc.jl:75-82 in one call: fm (D+1,T) STATIC features, row 1 power.
 * X = [fm[1,:]; push_delta(fm[2:end,:])] over the WHOLE matrix (bin/vc.jl:77-78), then vc(t, X) in chunks of length(t)
 * (src/common.jl:31-63), then fvpostf! (src/gv.jl:10-15) on rows 2..D+1 when sigma2 != NULL.  out (D+1,T).
 * The deltas are taken BEFORE chunking: frame kL+1 takes its delta from frame kL of the previous chunk, and only frames 1 and
 * T of the utterance keep the copy of the static value in the delta rows (src/datasets.jl:6-13); they are bit-identical to
 * vcmi_push_delta's.  Row 1 is passed through bit for bit.  Chunks are [kL+1, min((k+1)L, T)], L = length(t); afterwards
 * length(t) is the last chunk's length, as vcmi_vc_traj leaves it.
 * T = 0 is a no-op; sigma2 != NULL with T < 2: VCMI_ERR_DIM; length(t) < 1: VCMI_ERR_ARG.
 * This entry and the three that follow run on the calling thread's device: the device group of vcmi_set_devices is not used.
 * Device scratch of the four, per thread and grow-only: the converter input (2D,T) and the result (D,T); the host-pointer
 * entries add one staging matrix for fm, in which static input is converted IN PLACE (out has the shape of fm: the power row
 * never moves) -- (4D+1) T doubles for this entry; vcmi_vc_traj_postf and vcmi_vc_trajgv with is_static = 0 keep their
 * (D+1,T) result behind the (2D+1,T) input: (6D+2) T.  A host-pointer entry frees the three buffers on return when together
 * they exceed 256 MiB (kVcScratchKeepBytes, csrc/postf.hpp).  The converter handle's own per-frame workspace is that of
 * vcmi_traj_convert_batch_dev. */
int vcmi_vc_traj_static(vcmi_traj *t, const double *fm, int64_t T, const double *sigma2, double *out);
/* the same on DEVICE-RESIDENT matrices with leading dimensions (ldf >= the row count of dfm, ldo >= D+1; below:
 * VCMI_ERR_ARG), asynchronous on `stream` up to the status read that vcmi_traj_convert_batch_dev already does; dout must not
 * overlap dfm.  is_static = 0: dfm is (2D+1,T) (src/common.jl:31-63 as it stands); 1: dfm is (D+1,T) as above. */
int vcmi_vc_traj_dev(vcmi_traj *t, const double *dfm, int64_t ldf, int64_t T, int is_static, const double *sigma2,
                     double *dout, int64_t ldo, void *stream);

/* ---------------------------------------------------------------------------------------------
 * TrajectoryGVGMMMap -- src/trajectory_gmmmap.jl:114-189
 * ------------------------------------------------------------------------------------------- */
typedef struct vcmi_trajgv vcmi_trajgv;
/* TrajectoryGVGMMMap(tgmm, mu^v (D), Sigma^vv (D,D)) :118-129; keeps (does not own) the trajectory handle.
 * VCMI_ERR_ARG if a GV mean is negative (the @assert of :124), VCMI_ERR_NOT_PD if Sigma^vv is singular.
 * Every static dimension vcmi_traj_create accepts converts with GV.  2D <= 96: one wave per 16-row tile of Q_m with the tile's
 * k-steps in registers (traj_gv2_kernel; traj_gv_kernel where the frame permutation of the longest utterance does not fit LDS).
 * 2D > 96: traj_gvw_kernel -- several row tiles per wave, the k range in chunks of at most 16 k-steps through a 34 KB LDS image
 * whatever D is, Q_m read from the fragment image that vcmi_traj_create uploads for every dimension (no new buffer on the
 * handle); utterances whose (ceil(T/16) + M) 16 permutation slots exceed 1024 keep the permutation in the workspace.  Scratch of
 * the ascent, on the trajectory handle: per workgroup (one per utterance, at most one per compute unit) 3 D Tmax doubles (Q u and
 * r) and 8.5 Tmax + 16 more for the permutation, inside the workspace of the solve ((3D+1) D Tmax doubles per workgroup), which
 * is the larger of the two for every D >= 3.  D > 512 returns VCMI_ERR_ARG from the convert entries (the arg-max of the
 * trajectory converter ends at 2D = 320). */
int vcmi_trajgv_create(vcmi_traj *t, const double *muv, const double *sigmavv, vcmi_trajgv **out);
/* The same converter over a trajectory handle with DIAGONAL conditional precisions: vcmi_traj_set_precision(t, DIAG) or
 * vcmi_traj_create_bdiag.  Arguments and checks of vcmi_trajgv_create; VCMI_ERR_ARG if t's precision is not DIAG now.  The
 * handle goes to the same entries (vcmi_trajgv_convert, _batch, _batch_dev, vcmi_vc_trajgv, _dev, _batch, _batch_dev,
 * vcmi_trajgv_destroy) and converts only while t's precision is DIAG: after vcmi_traj_set_precision(t, FULL) every convert
 * entry returns VCMI_ERR_ARG before anything runs, and the handle is usable again after the switch back.  A handle of
 * vcmi_trajgv_create over the same t keeps refusing while t is DIAG.
 * With D^-1 = diag(q) the likelihood gradient is a three-point stencil per static dimension, (P y)_t = c0_t y_t +
 * c2_t y_{t-2} + c2_{t+2} y_{t+2} (csrc/traj_gv_band.hip): O(T D) per epoch, a Jacobi step on two y buffers.  traj_gvd_kernel
 * runs one workgroup per utterance with all epochs inside; as many of its five (T,D) arrays (y, second y, c2, c0, r) as fit
 * the 160 KB of LDS stay there across the epochs, chosen from D and the longest utterance of the call
 * (csrc/traj_band_plan.hpp), the rest is streamed: every T >= 2 converts.  An utterance's result does not depend on the batch
 * it came in.  Scratch on the trajectory handle: 5 D N doubles for the N frames of a call (the solver's D N and four more).
 * D > 512: VCMI_ERR_ARG.  Device groups: an ordinary DIAG converter shards as vcmi_trajgv_create's does; one of
 * vcmi_traj_create_bdiag converts on its own device. */
int vcmi_trajgv_create_diag(vcmi_traj *t, const double *muv, const double *sigmavv, vcmi_trajgv **out);
/* The same converter over a handle of vcmi_traj_create_bdiag[_windows] ONLY; any other t: VCMI_ERR_ARG naming vcmi_trajgv_create
 * and vcmi_trajgv_create_diag.  Arguments and checks of vcmi_trajgv_create_diag (a negative mu^v: VCMI_ERR_ARG; a singular
 * Sigma^vv: VCMI_ERR_NOT_PD).  Two windows: the handle is the one vcmi_trajgv_create_diag makes, every result bit for bit that
 * one's.  Three windows (vcmi_traj_create_bdiag_windows(b, T, 3), which vcmi_trajgv_create_diag keeps refusing): the likelihood
 * gradient is the five-point stencil of the pentadiagonal system the solver factorises,
 *   (P y)_t = c0_t y_t + c1_t y_{t-1} + c1_{t+1} y_{t+1} + c2_t y_{t-2} + c2_{t+2} y_{t+2}      (csrc/traj_gv_band_step.hpp),
 * a Jacobi step on two y buffers in traj_gvp_kernel (csrc/traj_gv_band.hip): one workgroup per utterance with all epochs
 * inside; as many of its six (T,D) arrays (y, second y, c1, c2, c0, r) as fit the 160 KB of LDS stay there across the epochs,
 * chosen from D and the longest utterance of the call (csrc/traj_band_plan.hpp), the rest is streamed: every T >= 2 converts, and
 * an utterance's result does not depend on the batch it came in.  Scratch on the trajectory handle: 5 D N doubles for the N
 * frames of a call, the first two on the solver's l1 and l2 (dead once the solve has run).  The three-window handle goes to
 * vcmi_trajgv_convert, _batch, _batch_dev (X (3D,T)) and to vcmi_vc_trajgv / vcmi_vc_trajgv_dev with is_static = 0 (fm (3D+1,T)),
 * with or without sigma2; is_static = 1 and vcmi_vc_trajgv_batch[_dev] stay VCMI_ERR_ARG ("three windows"), as for the plain
 * converter.  Converts on the device b was created on. */
int vcmi_trajgv_create_bdiag(vcmi_traj *t, const double *muv, const double *sigmavv, vcmi_trajgv **out);
int vcmi_trajgv_destroy(vcmi_trajgv *h);
/* fvconvert(tgv, X; epochs=100, alpha=1.0e-5) :139-168: trajectory solve, eq.(58) rescaling, then `epochs` steps of
 * y += alpha (omega (W'D^-1E - W'D^-1W y) + gvgrad(y)), all on the device.  X (2D,T) -> Y (D,T). */
int vcmi_trajgv_convert(vcmi_trajgv *h, const double *X, int64_t T, int epochs, double alpha, double *Y);
int vcmi_trajgv_convert_batch(vcmi_trajgv *h, int64_t n, const double *const *X, const int64_t *T, int epochs, double alpha,
                              double *const *Y);
int vcmi_trajgv_convert_batch_dev(vcmi_trajgv *h, int64_t n, const double *dX, const int64_t *x_off, const int64_t *T,
                                  int epochs, double alpha, double *dY, const int64_t *y_off, void *stream);
/* vc(c::TrajectoryConverter, fm) for TrajectoryGVGMMMap (src/common.jl:31-63): each chunk through
 * fvconvert(tgv, X; epochs, alpha) (src/trajectory_gmmmap.jl:139-168).  is_static = 0: fm is (2D+1,T); 1: fm is (D+1,T) STATIC
 * features and the deltas are taken over the whole matrix first (bin/vc.jl:75-78), as vcmi_vc_traj_static does.  sigma2 may be
 * NULL; otherwise fvpostf! (src/gv.jl:10-15) runs on rows 2..D+1 of the whole result.  A chunk of exactly one frame has no
 * variance: VCMI_ERR_DIM, before anything runs.  Afterwards length(h's trajectory converter) is the last chunk's length
 * (src/trajectory_gmmmap.jl:70-72,146).  Other rules, device and scratch: see vcmi_vc_traj_static / vcmi_vc_traj_dev. */
int vcmi_vc_trajgv(vcmi_trajgv *h, const double *fm, int64_t T, int is_static, int epochs, double alpha,
                   const double *sigma2, double *out);
int vcmi_vc_trajgv_dev(vcmi_trajgv *h, const double *dfm, int64_t ldf, int64_t T, int is_static, int epochs,
                       double alpha, const double *sigma2, double *dout, int64_t ldo, void *stream);

/* ---------------------------------------------------------------------------------------------
 * vc over a batch of utterances in one call (csrc/vc_batch.hip)
 * ------------------------------------------------------------------------------------------- */
/* THE RULE.  For utterances fm[0..n) of T[0..n) frames, out[u] is what vc(c_u, fm[u]) -- vcmi_vc_traj_static (is_static = 1,
 * fm[u] (D+1,T[u])) or vcmi_vc_traj_postf (is_static = 0, fm[u] (2D+1,T[u])) -- returns for a FRESH converter c_u equal to t
 * whose length is L = length(t) at entry:
 *   - every utterance is cut into chunks [kL+1, min((k+1)L, T[u])] with the same L;
 *   - static input gets its deltas over that utterance only, before chunking: only the utterance's own first and last frame
 *     keep the copy of the static value (src/datasets.jl:6-13);
 *   - the post-filter's mean and variance are taken over that utterance's converted frames only (src/gv.jl:10-15);
 *   - the power row is passed through bit for bit;
 *   - like the other batch entries, and unlike the single call, length(t) is left unchanged.
 * The chunks of all utterances go through ONE trajectory solve (the launch of vcmi_traj_convert_batch_dev), the two ends run as
 * segmented kernels over (utterance, tile) work lists made on the host; the filter's sums keep the order of the single call, so
 * an utterance's result carries the bits the single call computes.  vcmi_traj_set_em and vcmi_traj_set_precision are honoured
 * per chunk.
 * n = 0 is a no-op; T[u] = 0 is allowed and yields nothing for u.  Refused before anything is uploaded or launched, with every
 * output untouched and length(t) as it was: sigma2 with some T[u] = 1: VCMI_ERR_DIM; a GV converter with a one-frame chunk
 * (T[u] mod L = 1): VCMI_ERR_DIM; length(t) < 1, n < 0, T[u] < 0, a NULL matrix with T[u] > 0: VCMI_ERR_ARG; a GV converter
 * over a handle with EM switched on, or whose precision setting is not the one the GV handle was made for (vcmi_trajgv_create:
 * FULL, vcmi_trajgv_create_diag: DIAG): VCMI_ERR_ARG (as vcmi_vc_trajgv).
 * The entries run on the calling thread's device (the device group of vcmi_set_devices is not used), in the per-thread
 * scratch of the vcmi_vc_traj_static family under its rule (a host-pointer entry frees it on return above 256 MiB).  Footprint,
 * N = sum T: converter input and result, 3 D N doubles; the host-pointer entries add the staging matrix with the inputs and
 * the (D+1,N) results behind them -- (5D+2) N doubles in all for static input, (6D+2) N otherwise; the work lists (4 n + N / 128
 * words, with a filter 2 D n + D N / 2048 doubles more); and the handle's per-frame workspace of vcmi_traj_convert_batch_dev
 * over N frames.  A batch that does not fit is the caller's to slice. */
int vcmi_vc_traj_batch(vcmi_traj *t, int64_t n, const double *const *fm, const int64_t *T, int is_static, const double *sigma2,
                       double *const *out);
/* ... each chunk through fvconvert(tgv, X; epochs, alpha), as vcmi_vc_trajgv */
int vcmi_vc_trajgv_batch(vcmi_trajgv *h, int64_t n, const double *const *fm, const int64_t *T, int is_static, int epochs,
                         double alpha, const double *sigma2, double *const *out);
/* DEVICE-RESIDENT forms: utterance u lies dense ((D+1,T[u]) or (2D+1,T[u]), leading dimension = row count) at dfm + fm_off[u]
 * and its (D+1,T[u]) result dense at dout + out_off[u]; the offsets (in doubles, signed) and lengths are HOST arrays, as in
 * vcmi_traj_convert_batch_dev.  The input and output ranges must not overlap.  Asynchronous on `stream` up to the status read
 * the trajectory entries already do (the work lists are uploaded synchronously before the first launch). */
int vcmi_vc_traj_batch_dev(vcmi_traj *t, int64_t n, const double *dfm, const int64_t *fm_off, const int64_t *T, int is_static,
                           const double *sigma2, double *dout, const int64_t *out_off, void *stream);
int vcmi_vc_trajgv_batch_dev(vcmi_trajgv *h, int64_t n, const double *dfm, const int64_t *fm_off, const int64_t *T, int is_static,
                             int epochs, double alpha, const double *sigma2, double *dout, const int64_t *out_off, void *stream);

/* fvpostf(vs::VarianceScaling, src) -- src/gv.jl:10-21.  src, out (D,T), sigma2 (D); out may alias src.  D T doubles in the
 * same per-thread staging matrix, under the same rule (device-wide wait and release included). */
int vcmi_variance_scaling(const double *src, int D, int64_t T, const double *sigma2, double *out);
/* fvpostf! on a DEVICE-RESIDENT matrix (leading dimensions lds, ldo >= D; dout may be dsrc: in place), asynchronous on
 * `stream`; sigma2 (D) is a host vector.  Deterministic: every sum has a fixed order. */
int vcmi_variance_scaling_dev(const double *dsrc, int64_t lds, int D, int64_t T, const double *sigma2, double *dout,
                              int64_t ldo, void *stream);
/* diffgmm(params) -- src/diffgmm.jl:9-25 on joint parameters mu (2D,M), sigma (2D,2D,M); host arithmetic. */
int vcmi_diffgmm(const double *mu, const double *sigma, int Dj, int M, double *mu_out, double *sigma_out);

/* ---------------------------------------------------------------------------------------------
 * align_mcep and the joint training matrix -- src/align.jl:38-55, src/datasets.jl:52-98
 * ------------------------------------------------------------------------------------------- */
/* mc2e(mc, alpha, len) of MelGeneralizedCepstrums (third party; call site src/align.jl:48) for every column of
 * mc (D,T): energy of c2ir(freqt(mc, len-1, -alpha), len).  e (T).  2 <= fftlen <= 9600 (a frame's two length-len
 * vectors stay in the LDS; four frames per workgroup up to 2400, two up to 4800, one beyond); VCMI_ERR_ARG above that, here
 * and in vcmi_align_mcep / vcmi_parallel_dataset_dev with silence removal. */
int vcmi_mc2e(const double *mc, int D, int64_t T, double alpha, int fftlen, double *e);
/* align_mcep(src, tgt, alpha, fftlen; threshold=-14.0, remove_silence=true): align, then keep the columns whose
 * log(mc2e(src)) exceeds the threshold.  src (D,S), tgt (D,T); src_out, newtgt_out (D, up to S); *ncols kept. */
int vcmi_align_mcep(const double *src, int64_t S, const double *tgt, int64_t T, int D, double alpha, int fftlen,
                    double threshold, int remove_silence, double *src_out, double *newtgt_out, int64_t *ncols);
/* align_mcep of every pair followed by ParallelDataset(joint=true; diff, ignore0th, add_delta).X, left ON THE DEVICE
 * for the E-step: per pair drop row 1 (ignore0th), push_delta on the kept frames (add_delta), tgt - src (diff), vcat;
 * pairs concatenated in order.  do_align = 0 takes pairs that are already aligned (S == T).  dXY: device buffer of
 * Dj * capacity_frames doubles with capacity_frames >= sum(S), Dj = 2 (D - ignore0th)(1 + add_delta); *nframes
 * receives the number of columns written; counts (optional, host, n entries) the frames kept per pair. */
int vcmi_parallel_dataset_dev(int64_t n, const double *const *src, const int64_t *S, const double *const *tgt,
                              const int64_t *T, int D, int do_align, double alpha, int fftlen, double threshold,
                              int remove_silence, int ignore0th, int add_delta, int diff, double *dXY,
                              int64_t capacity_frames, int64_t *nframes, int64_t *counts);

/* ---------------------------------------------------------------------------------------------
 * Spectral envelopes into and out of vc: sp2mc, mc2sp, mc2b of MelGeneralizedCepstrums (third party)
 * ------------------------------------------------------------------------------------------- */
/* sp2mc(sp, order, alpha) -- call sites test/vc.jl:16, bin/vc.jl:71, bin/mcep.jl:50.  sp (K,T) power spectra (K = fftlen/2+1,
 * 2 <= K <= 4097), mc (order+1,T), 1 <= order+1 <= 256, |alpha| < 1: per column c = irfft(log sp, 2(K-1)), c[0] /= 2,
 * mc = freqt(c, order, alpha) over all 2(K-1) entries.  VCMI_ERR_ARG if an entry of sp is not positive and finite
 * (Julia's log throws); the check rides on the kernel's own reads.
 * mc2sp(mc, alpha, fftlen) -- call sites test/vc.jl:28, bin/vc.jl:87.  mc (D,T), 1 <= D <= 256, 2 <= fftlen <= 8193 (odd
 * lengths included: the reference passes 2 size(sp,1) - 1), sp (fftlen/2+1,T): per column c = freqt(mc, fftlen/2, -alpha),
 * c[0] *= 2, sp = exp(real(rfft(symmetric vector of c))).
 * mc2b(mc, alpha) -- call sites test/diffvc.jl:33, bin/diffvc.jl:83.  mc, b (D,T): b[D-1] = mc[D-1],
 * b[i] = mc[i] - alpha b[i+1].
 * Host pointers: per-thread scratch, staged upload, kernel, download (like vcmi_mc2e).  `_dev` variants take DEVICE-RESIDENT
 * matrices with leading dimensions (>= the column length), are asynchronous on `stream` and do NOT check the values of
 * their input (a non-positive power gives NaN or -inf).  All six run on the calling thread's device: the device group of
 * vcmi_set_devices is not used.  T = 0 is a no-op. */
int vcmi_sp2mc(const double *sp, int K, int64_t T, int order, double alpha, double *mc);
int vcmi_sp2mc_dev(const double *dsp, int64_t lds, int K, int64_t T, int order, double alpha,
                   double *dmc, int64_t ldm, void *stream);
int vcmi_mc2sp(const double *mc, int D, int64_t T, double alpha, int fftlen, double *sp);
int vcmi_mc2sp_dev(const double *dmc, int64_t ldm, int D, int64_t T, double alpha, int fftlen,
                   double *dsp, int64_t lds, void *stream);
int vcmi_mc2b(const double *mc, int D, int64_t T, double alpha, double *b);
int vcmi_mc2b_dev(const double *dmc, int64_t ldm, int D, int64_t T, double alpha,
                  double *db, int64_t ldb, void *stream);

/* GVDataset(path; ignore0th, add_delta, nmax) from in-memory feature matrices -- src/datasets.jl:134-183 (the file loop
 * is the caller's): per utterance tgt = fm[i] (D,T[i]) without row 1 (ignore0th), with push_delta (add_delta);
 * gv = var(tgt, 2) (corrected, Julia's default); an utterance whose variance has a NaN (T = 1) is skipped as the
 * reference does.  out: (Dout, n) column-major, Dout = (D - ignore0th)(1 + add_delta), the kept utterances' columns in
 * order; *nkept = how many.  Host-side helper (O(D sum T), shared out over the library's host threads). */
int vcmi_gv_dataset(int64_t n, const double *const *fm, const int64_t *T, int D, int ignore0th, int add_delta, double *out,
                    int64_t *nkept);

#ifdef __cplusplus
}
#endif
#endif /* VCMI_H */
