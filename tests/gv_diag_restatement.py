"""numpy.longdouble restatement of ONE EPOCH of the global-variance ascent over DIAGONAL conditional precisions
(DiagTrajectoryGVGMMMap, vcmi_trajgv_create_diag; csrc/traj_gv_band.hip: traj_gvd_kernel) -- test infrastructure, numpy only.

Two statements of the same epoch  y <- y + alpha (lik + gv)(y):

  dense     tests/gv_restatement.py's gradient_terms / gv_term / step_bar, IMPORTED AND USED UNCHANGED, on a Pieces-shaped object
            (DiagPieces) whose per-mixture precision Dinv[m] is diag(q_m) embedded in a (2D,2D) matrix: the reference's own
            statement, W as its stencil or as the matrix np_oracle.constructW builds;
  stencil   what the kernel evaluates, per static dimension:
                (P y)_t = c0_t y_t + c2_t y_{t-2} + c2_{t+2} y_{t+2},   c0_t = p_s(t) + p_d(t-1)/4 + p_d(t+1)/4,  c2_t = -p_d(t-1)/4
                r_t     = g_s(t) + g_d(t-1)/2 - g_d(t+1)/2,             [p_s ; p_d] = q[mhat_t],  g_t = q[mhat_t] (.) E_t
            a p_d of a frame outside the utterance absent everywhere, a y_{t+-2} outside the utterance absent while the
            p_d(t-+1)/4 y_t of the existing neighbour frame stays (stencil_terms);  tests/test_gv_diag_restatement_host.py shows
            the two agree to 1e-15.

The pieces come from a cross-diagonal model (tests/traj_bdiag_restatement.py: BdiagTrajectory) or from a full model in diagonal
mode (tests/traj_diag_restatement.py: DiagTrajectory).

The magnitude of E.  gradient_terms takes E_t as given and bounds the rounding of r = W' D^-1 E by K 2^-53 W'|D^-1||E|.  The device
does not receive E: it SUMS it, and so does the restatement's numpy, each in its own order:
    cross-diagonal   E_k = mu^y_k + a_k (x_k - mu^x_k)            three roundings; off by <= 3 2^-53 (|mu^y| + |a| |x - mu^x|)_k
    dense mode       E   = b + A x,  b = mu^y - A mu^x            a chain of 2D + 1 terms; off by <= (2D + 2) 2^-53 (|b| + |A| |x|)
Where the terms cancel, |E| is far below those magnitudes and two right evaluations of E differ by more than any multiple of
2^-53 |E|: E's rounding is relative to the TERMS.  So the bar is fed  Emag = |mu^y| + |a| |x - mu^x|  (cross-diagonal) or
|b| + |A| |x|  (dense mode) in place of |E| (lik_magnitude), and in the dense mode the chain length K grows by 2D, the length of
the sum A x that sits in front of the 3 * 2D of the product (step_bar_diag).  With diag(q) the product q (.) u is ONE term, not
2D: the kernel's chain is shorter than the 3 * 2D the bar counts, the bar is an upper bound and stays as gv_restatement states it.

MUTANTS: gv_restatement.MUTANTS without the tile mutant (the kernel has no tiles), evaluated by gradient_terms, and three of the
stencil: the Gauss-Seidel update (y_{t-2} from the NEW epoch: an in-place update reads what another thread has already
written), c2 from the wrong neighbour (p_d(t+1) for p_d(t-1)), and the boundary p_d(t-+1)/4 y_t dropped together with the absent
y_{t-+2}.

Arrays follow oracle/np_oracle.py: [frame, feature]."""
import functools

import numpy as np

import gv_restatement as gr
import traj_bdiag_restatement as tb
import traj_diag_restatement as td
import traj_full_restatement as tf
from em_bdiag_restatement import bdiag_model
from gv_restatement import EPS, LD
from oracle import np_oracle as npo

DENSE_MUTANTS = tuple(m for m in gr.MUTANTS if m != "tile_last_frame_mixture")
STENCIL_MUTANTS = ("gauss_seidel", "c2_wrong_neighbour", "boundary_diagonal_dropped")
MUTANTS = DENSE_MUTANTS + STENCIL_MUTANTS


# ------------------------------------------------------------------------------------------------ launch rule
# csrc/traj_band_plan.hpp, restated: of the kernel's five (T,D) arrays (y, second y, c2, c0, r) as many as fit 160 KB - 256 B of
# LDS beside the two reduction rows of 512 doubles and mean, var, coef stay resident; fewer than two: none (the streamed form)
GVD_THREADS = 512
LDS_LIMIT = 160 * 1024 - 256


def gvd_resident(D, Tmax):
    """0 (streamed), 2, 3, 4 or 5 arrays in LDS for a call whose longest utterance has Tmax frames"""
    fit = (LDS_LIMIT - (2 * GVD_THREADS + 3 * D) * 8) // (Tmax * D * 8)
    return 5 if fit >= 5 else (int(fit) if fit >= 2 else 0)


# ------------------------------------------------------------------------------------------------ pieces
class DiagPieces:
    """What gv_restatement.gradient_terms takes (mhat (T,) 1-based, E (T,2D), Dinv (M,2D,2D), muv (D,), pv (D,D), T, D), with
    Dinv[m] = diag(q_m); also q (M,2D), Emag (T,2D) and the chain length the E sum adds (0 or 2D)."""

    def __init__(self, mhat, E, Emag, q, muv, Sigvv, extra_chain):
        self.T, self.D = E.shape[0], E.shape[1] // 2
        self.mhat, self.E, self.Emag, self.q = np.asarray(mhat), E, Emag, q
        self.Dinv = np.stack([np.diag(qm) for qm in q])
        self.muv = np.asarray(muv, dtype=np.float64)
        self.pv = np.linalg.inv(np.asarray(Sigvv, dtype=np.float64))
        self.extra_chain = extra_chain

    def with_magnitude_as_E(self):
        """the same pieces with Emag in place of E: gradient_terms' lik_mag of these is the magnitude the bar is fed"""
        p = object.__new__(DiagPieces)
        p.__dict__.update(self.__dict__)
        p.E = self.Emag
        return p


def pieces_bdiag(bt, X, muv, Sigvv, mhat=None):
    """bt: traj_bdiag_restatement.BdiagTrajectory; X (T,2D)"""
    m = (bt.mhat(X) if mhat is None else np.asarray(mhat)) - 1
    mux, muy, a = bt.mux.T[m], bt.muy.T[m], bt.a.T[m]
    adx = a * (X - mux)
    return DiagPieces(m + 1, muy + adx, np.abs(muy) + np.abs(adx), np.ascontiguousarray(bt.q.T), muv, Sigvv, 0)


def pieces_dense(dt, X, muv, Sigvv):
    """dt: traj_diag_restatement.DiagTrajectory (a full model in diagonal mode); X (T,2D)"""
    g = dt.g
    mhat = g.predict(X)
    E = np.stack([g.muy[m - 1] + g.A[m - 1] @ (X[t] - g.mux[m - 1]) for t, m in enumerate(mhat)])
    Emag = np.stack([np.abs(g.muy[m - 1] - g.A[m - 1] @ g.mux[m - 1]) + np.abs(g.A[m - 1]) @ np.abs(X[t]) for t, m in enumerate(mhat)])
    return DiagPieces(mhat, E, Emag, dt.q, muv, Sigvv, X.shape[1])


# ------------------------------------------------------------------------------------------------ the stencil
def _coefficients(p, mutant=None):
    """c0, c2, r, r_mag (T,D) long double; c2_t is the coefficient of y_{t-2} (zero for t < 2)"""
    T, D = p.T, p.D
    qt = p.q.astype(LD)[p.mhat - 1]
    ps, pd = qt[:, :D], qt[:, D:]
    g, gm = qt * p.E.astype(LD), qt * p.Emag.astype(LD)
    c0 = ps.copy()
    c0[1:] += pd[:-1] / 4
    c0[:-1] += pd[1:] / 4
    c2 = np.zeros((T, D), dtype=LD)
    c2[2:] = -pd[1:-1] / 4
    if mutant == "c2_wrong_neighbour":        # P[t,t-2] from p_d(t+1) (absent for the last frame)
        c2[2:] = 0
        c2[2:T - 1] = -pd[3:] / 4
    if mutant == "boundary_diagonal_dropped" and T >= 2:   # frames 1 and T-2 lose the p_d/4 y_t of the neighbour whose far side is absent
        c0[1] -= pd[0] / 4
        c0[T - 2] -= pd[T - 1] / 4
    r, rmag = g[:, :D].copy(), gm[:, :D].copy()
    r[1:] += g[:-1, D:] / 2
    r[:-1] -= g[1:, D:] / 2
    rmag[1:] += gm[:-1, D:] / 2
    rmag[:-1] += gm[1:, D:] / 2
    return c0, c2, r, rmag


def stencil_terms(p, y, mutant=None):
    """(P y, r) (T,D) long double in the tridiagonal form"""
    c0, c2, r, _ = _coefficients(p, mutant)
    y = np.asarray(y, dtype=LD)
    Py = c0 * y
    Py[2:] += c2[2:] * y[:-2]
    Py[:-2] += c2[2:] * y[2:]
    return Py, r


def lik_magnitude(p, y):
    """omega (W'|D^-1| Emag + W'|D^-1||W||y|) in the tridiagonal form: gradient_terms' lik_mag with Emag for |E|"""
    c0, c2, _, rmag = _coefficients(p)
    ay = np.abs(np.asarray(y, dtype=LD))
    Pa = c0 * ay
    Pa[2:] += np.abs(c2[2:]) * ay[:-2]
    Pa[:-2] += np.abs(c2[2:]) * ay[2:]
    return (rmag + Pa) / (2 * p.T)


def gradient(p, y, mutant=None):
    """(lik, gv) (T,D) long double; the dense mutants through gv_restatement.gradient_terms, the stencil's own here"""
    if mutant in DENSE_MUTANTS:
        lik, gv, _, _ = gr.gradient_terms(p, y, mutant, mags=False)
        return lik, gv
    Py, r = stencil_terms(p, y, mutant if mutant != "gauss_seidel" else None)
    return (r - Py) / (2 * p.T), gr.gv_term(p.pv, p.muv, y)[0]


def step(p, y, alpha, mutant=None):
    """y + alpha (lik + gv)(y), long double.  gauss_seidel: frame t takes y_{t-2} from the new epoch, y_{t+2} from the old"""
    y = np.asarray(y, dtype=LD)
    if mutant != "gauss_seidel":
        lik, gv = gradient(p, y, mutant)
        return y + LD(alpha) * (lik + gv)
    c0, c2, r, _ = _coefficients(p)
    gv = gr.gv_term(p.pv, p.muv, y)[0]
    new = y.copy()
    T = p.T
    for t in range(T):
        Py = c0[t] * y[t]
        if t >= 2:
            Py = Py + c2[t] * new[t - 2]
        if t + 2 < T:
            Py = Py + c2[t + 2] * y[t + 2]
        new[t] = y[t] + LD(alpha) * ((r[t] - Py) / (2 * T) + gv[t])
    return new


def chain_length(p):
    return gr.chain_length(p.D, p.T) + p.extra_chain


def step_bar_diag(p, alpha, y_n, y_n1, gv_mag):
    """gv_restatement.step_bar fed lik_magnitude (Emag for |E|), its K raised by the chain of the E sum"""
    bar = gr.step_bar(p.D, p.T, alpha, y_n, y_n1, lik_magnitude(p, y_n), gv_mag)
    return bar * (LD(chain_length(p)) / gr.chain_length(p.D, p.T))


def ascent(p, y0, epochs, alpha, keep=()):
    y = np.asarray(y0, dtype=LD)
    kept = {}
    for n in range(epochs + 1):
        if n in keep:
            kept[n] = y.copy()
        if n < epochs:
            y = step(p, y, alpha)
    return y, kept


# ------------------------------------------------------------------------------------------------ the step-visible inputs
# Both converter kinds at the shapes of tests/test_gpu_gv_diag.py.  Frames follow tests/gv_restatement.py: a PRESCRIBED mixture
# sequence (traj_full_restatement.sequence) and X_t = the source mean of mixture s_t + noise, which the arg-max takes with a clear
# margin (asserted on the host) -- the device and the restatement then work on the same mhat.
#   dense   traj_full_restatement.model(700 + D, D, M) (synth_model, lam_lo = 0.1: mixtures conditioned <= 10, so the device's
#           and numpy's inverses of the model preparation differ far below the running error) in diagonal mode, frames
#           traj_full_restatement.utterance;
#   bdiag   em_bdiag_restatement.bdiag_model(900 + D, 4D, M, sep = BDIAG_SEP): well separated means, X_t = mu^x[s_t] +
#           0.3 sqrt(vx[s_t]) N(0, I).
# GV statistics: gv_restatement.gv_stats (asymmetric covariance) on the plain trajectory of the group's `cycle` utterance of
# STATS_T frames, the covariance times the case's cov_scale.  alpha and cov_scale per case: a grid search on the CPU (alpha in
# {1, 3} 10^k, scale in 10^k: tools/gv_diag_case_search.py) against gv_restatement's conditions -- both summands >= 0.2 of every
# checked step for n >= 1, the step >= 1e-5 of max |y|, y finite and within 10 max |y_0| -- never against the kernel.
BDIAG_SEP = 6.0
NOISE = 0.3
STATS_T = 50
N_FULL, N_SHORT = gr.N_FULL, gr.N_SHORT


class Case:
    def __init__(self, kind, D, M, seq, T, alpha, cov_scale, ns=N_FULL):
        self.kind, self.D, self.M, self.seq, self.T, self.alpha, self.cov_scale, self.ns = kind, D, M, seq, T, alpha, cov_scale, ns

    @property
    def id(self):
        return f"{self.kind}-D{self.D}-M{self.M}-T{self.T}"


@functools.lru_cache(maxsize=None)
def group(kind, D, M):
    """(model, restatement converter, mu_v, Sigma_vv at scale 1) of a (kind, D, M) group"""
    if kind == "bdiag":
        mdl = bdiag_model(900 + D, 4 * D, M, sep=BDIAG_SEP)
        conv = tb.BdiagTrajectory(*mdl)
    else:
        mdl = tf.model(tf.MODEL_SEED + D, D, M)
        conv = td.DiagTrajectory(*mdl)
    Xs, s = utterance(kind, mdl, D, M, "cycle", STATS_T)
    muv, Sv = gr.gv_stats(np.random.default_rng(D), plain_trajectory(kind, conv, Xs, s))
    for a in (muv, Sv):
        a.setflags(write=False)
    return mdl, conv, muv, Sv


def utterance(kind, mdl, D, M, seq, T):
    """(X (T,2D), s 1-based)"""
    if kind == "dense":
        return tf.utterance(mdl, D, M, seq, T, 1)
    rng = np.random.default_rng([2, D, T])
    s = tf.sequence(seq, M, T, rng)
    _, mu, cov = mdl
    return mu[:2 * D, s].T + NOISE * np.sqrt(cov[:2 * D, s].T) * rng.standard_normal((T, 2 * D)), s + 1


def plain_trajectory(kind, conv, X, s):
    """the restatement's tridiagonal solve of the plain trajectory, on the prescribed sequence"""
    if kind == "bdiag":
        return conv.tridiag(X, s)[0]
    return conv.tridiag(X)[0]


@functools.lru_cache(maxsize=None)
def _inputs(kind, D, M, seq, T, cov_scale):
    mdl, conv, muv, Sv = group(kind, D, M)
    X, s = utterance(kind, mdl, D, M, seq, T)
    Sv = Sv * cov_scale
    p = pieces_bdiag(conv, X, muv, Sv) if kind == "bdiag" else pieces_dense(conv, X, muv, Sv)
    y0 = npo.variance_scaling(plain_trajectory(kind, conv, X, s), muv)
    for a in (X, s, Sv, y0):
        a.setflags(write=False)
    return dict(model=mdl, conv=conv, X=X, s=s, muv=muv, Sv=Sv, pieces=p, y0=y0)


def inputs(case):
    """model, restatement converter, X (T,2D), the prescribed sequence s (1-based), GV statistics, DiagPieces and the eq. (58)
    start of a case -- made once, never written to"""
    return _inputs(case.kind, case.D, case.M, case.seq, case.T, case.cov_scale)


# (D, M, seq, T, ns): D = 12 -- T = 2, 3: no +-2 neighbour at all; 4, 5: one; 16, 17, 50: all boundary combinations inside a
# longer utterance; D = 33: a row one past 32 lanes; D = 40: the ordinary shape, streamed (one array is 96 KB); D = 59: 2D > 96,
# the wide kernel's range in the full mode; D = 64: 2D = 128, the cross-diagonal limit; M = 256: many mixtures; and at D = 12 the
# launch rule's edges: T = 323 / 324 (five arrays resident / four), 403 / 404 (four / three), 538 / 539 (three / two) and
# 807 / 808 (two -- the last T of an LDS-resident form -- / streamed)
SHAPES = ([(12, 4, "cycle", T, N_FULL) for T in (2, 3, 4, 5, 16, 17, 50)] +
          [(33, 3, "rand", 64, N_FULL), (33, 3, "rand", 65, N_FULL), (40, 8, "runs", 300, N_FULL), (59, 4, "cycle", 70, N_FULL),
           (64, 5, "cycle", 33, N_FULL), (4, 256, "cycle", 70, N_FULL)] +
          [(12, 4, "runs", T, N_SHORT) for T in (324, 404, 539, 807, 808)])
# one fvconvert_batch call, both sides of the launch rule: the batch runs streamed (its longest member), the members alone run
# with two and with four arrays resident
BATCH_TS = (808, 807, 324)

# (alpha, cov_scale) per (kind, D, M, T), and per kind for the batch: what tools/gv_diag_case_search.py prints
SETTINGS = {
    ("bdiag", 12, 4, 2): (0.1, 10), ("bdiag", 12, 4, 3): (0.0003, 0.01), ("bdiag", 12, 4, 4): (0.0003, 0.01),
    ("bdiag", 12, 4, 5): (0.3, 10), ("bdiag", 12, 4, 16): (0.1, 1), ("bdiag", 12, 4, 17): (0.1, 1),
    ("bdiag", 12, 4, 50): (0.003, 0.01), ("bdiag", 33, 3, 64): (1, 10), ("bdiag", 33, 3, 65): (1, 10),
    ("bdiag", 40, 8, 300): (10, 10), ("bdiag", 59, 4, 70): (1, 10), ("bdiag", 64, 5, 33): (0.001, 0.01),
    ("bdiag", 4, 256, 70): (0.003, 0.001), ("bdiag", 12, 4, 324): (3, 1), ("bdiag", 12, 4, 404): (3, 1),
    ("bdiag", 12, 4, 539): (0.03, 0.01), ("bdiag", 12, 4, 807): (30, 10), ("bdiag", 12, 4, 808): (30, 10),
    ("dense", 12, 4, 2): (0.0003, 0.01), ("dense", 12, 4, 3): (0.0003, 0.01), ("dense", 12, 4, 4): (0.3, 10),
    ("dense", 12, 4, 5): (0.3, 10), ("dense", 12, 4, 16): (1, 10), ("dense", 12, 4, 17): (1, 10),
    ("dense", 12, 4, 50): (3, 10), ("dense", 33, 3, 64): (3, 10), ("dense", 33, 3, 65): (3, 10),
    ("dense", 40, 8, 300): (30, 10), ("dense", 59, 4, 70): (1, 1), ("dense", 64, 5, 33): (3, 10),
    ("dense", 4, 256, 70): (10, 10), ("dense", 12, 4, 324): (100, 100), ("dense", 12, 4, 404): (30, 10),
    ("dense", 12, 4, 539): (100, 100), ("dense", 12, 4, 807): (0.1, 0.01), ("dense", 12, 4, 808): (0.1, 0.01),
}
BATCH_SETTING = {"bdiag": (3, 1), "dense": (30, 10)}


def _cases():
    out = []
    for kind in ("bdiag", "dense"):
        for D, M, seq, T, ns in SHAPES:
            alpha, scale = SETTINGS[(kind, D, M, T)]
            out.append(Case(kind, D, M, seq, T, alpha, scale, ns))
    return out


def _batch_cases():
    return {kind: [Case(kind, 12, 4, "runs" if T > 100 else "cycle", T, *BATCH_SETTING[kind], N_SHORT) for T in BATCH_TS]
            for kind in ("bdiag", "dense")}


CASES = _cases()
BATCH_CASES = _batch_cases()
ALL_CASES = CASES + BATCH_CASES["bdiag"] + BATCH_CASES["dense"]
