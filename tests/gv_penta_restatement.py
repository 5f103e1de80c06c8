"""numpy.longdouble restatement of ONE EPOCH of the global-variance ascent over a converter with THREE windows (static + delta +
delta-delta): BlockDiagTrajectoryGVGMMMap over BlockDiagTrajectoryGMMMap(g, T, windows=3), vcmi_trajgv_create_bdiag;
csrc/traj_gv_band.hip: traj_gvp_kernel -- test infrastructure, numpy only.

Notation of tests/traj_penta_restatement.py: q[mhat_t] = [p_s ; p_d ; p_a], g_t = q[mhat_t] (.) E_t = [g_s ; g_d ; g_a].  Two
statements of the same epoch  y <- y + alpha (lik + gv)(y),  lik = omega (W'D^-1E - W'D^-1W y),  omega = 1/(2T):

  dense     through the explicit W of traj_penta_restatement.construct_w (3DT x DT) and D^-1 = diag(q[mhat_t]) over all frames
            (gradient_terms(dense=True); small cases), or with W and W' applied as operators (the same rows, any size -- the form
            that carries the mutants of gv_restatement.MUTANTS that apply here);
  stencil   what the kernel evaluates, per static dimension the five-point form
                c0_t = P[t,t]   = p_s(t) + p_d(t-1)/4 + p_d(t+1)/4 + p_a(t-1) + 4 p_a(t) + p_a(t+1)
                c1_t = P[t-1,t] = -2 p_a(t-1) - 2 p_a(t)                 (0 for t < 1)
                c2_t = P[t-2,t] = -p_d(t-1)/4 + p_a(t-1)                 (0 for t < 2)
                r_t  = g_s(t) + g_d(t-1)/2 - g_d(t+1)/2 + g_a(t-1) - 2 g_a(t) + g_a(t+1)
                (P y)_t = c0_t y_t + c1_t y_{t-1} + c1_{t+1} y_{t+1} + c2_t y_{t-2} + c2_{t+2} y_{t+2}
            a p or g of a frame outside the utterance absent, a y_{t+-1}, y_{t+-2} outside the utterance with weight 0 while what
            the existing neighbour frames add to c0 stays (stencil_terms).
Both take the GV term from gv_restatement.gv_term, imported and used unchanged.  tests/test_gv_penta_restatement_host.py shows
that the two agree to 1e-15.

The bar of a step is gv_restatement.step_bar's,  K 2^-53 (|y_n| + |y_{n+1}| + alpha (lik_mag + gv_mag)), with two changes that
tests/gv_diag_restatement.py derives for the two-window converter and that carry over word for word:
  - the magnitude of E.  The device does not receive E, it sums  E_k = mu^y_k + a_k (x_k - mu^x_k)  in its own order; where the
    terms cancel, two right evaluations differ by a multiple of 2^-53 of the TERMS, not of |E|.  lik_mag is therefore fed
    Emag = |mu^y| + |a| |x - mu^x| in place of |E| (lik_magnitude, the five-point form of  omega (W'|D^-1| Emag + |W|'|D^-1||W||y|));
  - the same holds inside P: c2_t = -p_d(t-1)/4 + p_a(t-1) is a DIFFERENCE, so its share of the magnitude is p_d(t-1)/4 + p_a(t-1),
    which is what |W|'|D^-1||W| holds at (t-2,t); c0 and c1 are sums of terms of one sign and are their own magnitudes.
The chain length: gv_restatement.chain_length counts 3 * 2D for the product Q u with the stencil of W on either side of it, u of
dimension 2D.  Here u = W y has dimension 3D, so K = 3 * 3D + T + D + 16 (chain_length below); T for the moments, D for the
Sigma_vv^-1 product and the constant are unchanged.  With diag(q) the product q (.) u is one term, not 3D: the kernel's chain
(eleven terms in r - P y) is far shorter than the bar counts.  The bar is an upper bound and is not tightened.

The whole ascent (increment_bar): gv_restatement.increment_bar's form, cond 2^-53 c / (max |y_init - y_ml| / max |y|) with
c = 64 * 2 * 2 * s * max |y_init - y_ml| / max |inc|, carries over with cond the largest 2-norm condition number of the
pentadiagonal matrices (traj_penta_restatement.banded): each of its factors is a statement about a symmetric positive definite
system solved backward-stably (64 cond 2^-53 is the parity bar of tests/traj_penta_restatement.py; two solutions differ by
twice that), about eq. (58) (s) and about a non-expanding ascent (|A - I| <= 2); none is about the bandwidth.  The factor rho of
the solver's own bound (the right-hand side summed from cancelling terms) multiplies it, as it does there.

MUTANTS: the mutants of gv_restatement.MUTANTS that apply (all but the tile mutant: the kernel has no tiles), evaluated in the
operator form, and seven of the stencil: the Gauss-Seidel update (y_{t-1}, y_{t-2} from the NEW epoch), c1 from the wrong
neighbour (P[t,t+1] for P[t-1,t]), c2 from the wrong neighbour (frame t+1 for t-1), c2 without its p_a term (the two-window
coefficient), r without its delta-delta term, and the boundary contributions to c0 dropped together with the absent y_{t-+2}.

Arrays follow oracle/np_oracle.py: [frame, feature]."""
import functools

import numpy as np

import gv_restatement as gr
import traj_full_restatement as tf
import traj_penta_restatement as tp
from em_bdiag_restatement import bdiag_model
from gv_restatement import EPS, LD
from oracle import np_oracle as npo

DENSE_MUTANTS = tuple(m for m in gr.MUTANTS if m != "tile_last_frame_mixture")
GV_MUTANTS = ("gv_dropped", "two_over_T_minus_1", "uncorrected_variance", "pv_diagonal", "pv_not_transposed", "wrong_mean")
STENCIL_MUTANTS = ("gauss_seidel", "c1_wrong_neighbour", "c2_wrong_neighbour", "c2_without_pa", "r_delta_delta_dropped",
                   "boundary_diagonal_dropped")
MUTANTS = DENSE_MUTANTS + STENCIL_MUTANTS

# ------------------------------------------------------------------------------------------------ launch rule
# csrc/traj_band_plan.hpp, restated: of the kernel's six (T,D) arrays (y, second y, c1, c2, c0, r) as many as fit 160 KB - 256 B of
# LDS beside the two reduction rows of 512 doubles and mean, var, coef stay resident; fewer than two: none (the streamed form)
GVP_THREADS = 512
LDS_LIMIT = 160 * 1024 - 256
GVP_ARRAYS = 6


def gvp_resident(D, Tmax):
    """0 (streamed), 2 .. 6 arrays in LDS for a call whose longest utterance has Tmax frames"""
    fit = (LDS_LIMIT - (2 * GVP_THREADS + 3 * D) * 8) // (Tmax * D * 8)
    return GVP_ARRAYS if fit >= GVP_ARRAYS else (int(fit) if fit >= 2 else 0)


def gvp_ws_doubles(nframes, D, with_gv):
    """workspace of a three-window call: the solver's l1, l2; with GV five arrays, the first two on l1 and l2"""
    return (5 if with_gv else 2) * nframes * D


# ------------------------------------------------------------------------------------------------ pieces
class PentaPieces:
    """mhat (T,) 1-based, E (T,3D), Emag (T,3D), q (M,3D), muv (D,), pv = Sigma_vv^-1 (D,D) as the oracle takes it"""

    def __init__(self, mhat, E, Emag, q, muv, Sigvv):
        self.T, self.D = E.shape[0], E.shape[1] // 3
        self.mhat, self.E, self.Emag, self.q = np.asarray(mhat), E, Emag, q
        self.muv = np.asarray(muv, dtype=np.float64)
        self.pv = np.linalg.inv(np.asarray(Sigvv, dtype=np.float64))

    def with_magnitude_as_E(self):
        p = object.__new__(PentaPieces)
        p.__dict__.update(self.__dict__)
        p.E = self.Emag
        return p


def pieces(bt, X, muv, Sigvv, mhat=None):
    """bt: traj_penta_restatement.PentaTrajectory; X (T,3D)"""
    m = (bt.mhat(X) if mhat is None else np.asarray(mhat)) - 1
    mux, muy, a = bt.mux.T[m], bt.muy.T[m], bt.a.T[m]
    adx = a * (X - mux)
    return PentaPieces(m + 1, muy + adx, np.abs(muy) + np.abs(adx), np.ascontiguousarray(bt.q.T), muv, Sigvv)


# ------------------------------------------------------------------------------------------------ the dense statement
def _W(y, D, sign=1, dw=0.5):
    """u = W y (T,3D): [y_t ; (y_{t+1} - y_{t-1}) / 2 ; y_{t-1} - 2 y_t + y_{t+1}], a missing neighbour contributing nothing.
    sign = -1: |W| |y| (every weight positive)"""
    T = y.shape[0]
    nxt, prv = np.zeros_like(y), np.zeros_like(y)
    nxt[:-1] = y[1:]
    prv[1:] = y[:-1]
    u = np.zeros((T, 3 * D), dtype=LD)
    u[:, :D] = y
    u[:, D:2 * D] = dw * nxt - sign * dw * prv
    u[:, 2 * D:] = prv - sign * 2 * y + nxt
    return u


def _Wt(v, D, sign=1, drop=None):
    """W' v (T,D): vs_t + vd_{t-1}/2 - vd_{t+1}/2 + va_{t-1} - 2 va_t + va_{t+1}.  drop = "first" / "last": the mutant that loses the
    one delta neighbour frame 0 / frame T-1 has."""
    T = v.shape[0]
    vs, vd, va = v[:, :D], v[:, D:2 * D], v[:, 2 * D:]
    dprv, dnxt, aprv, anxt = (np.zeros_like(vs) for _ in range(4))
    dprv[1:] = 0.5 * vd[:-1]
    dnxt[:-1] = 0.5 * vd[1:]
    aprv[1:] = va[:-1]
    anxt[:-1] = va[1:]
    if drop == "first":
        dnxt[0] = 0
    if drop == "last":
        dprv[T - 1] = 0
    return vs + dprv - sign * dnxt + aprv - sign * 2 * va + anxt


def gradient_terms(p, y, mutant=None, dense=False, mags=True):
    """(lik, gv, lik_mag, gv_mag), each (T,D) long double: gv_restatement.gradient_terms for three windows and D^-1 = diag(q).
    dense: W as traj_penta_restatement.construct_w builds it (no mutant); otherwise W and W' as operators."""
    assert mutant is None or mutant in DENSE_MUTANTS, mutant
    T, D = p.T, p.D
    y = np.asarray(y, dtype=LD)
    assert y.shape == (T, D)
    qt = p.q.astype(LD)[p.mhat - 1]               # (T,3D)
    E = p.E.astype(LD)
    omega = LD(1) / (T if mutant == "omega_one_over_T" else 2 * T)
    if dense:
        assert mutant is None
        W = tp.construct_w(D, T).astype(LD)
        dq = qt.ravel()
        lik = (omega * (W.T @ (dq * E.ravel()) - W.T @ (dq * (W @ y.ravel())))).reshape(T, D)
        aW = np.abs(W)
        lik_mag = (omega * (aW.T @ (dq * np.abs(E).ravel()) + aW.T @ (dq * (aW @ np.abs(y).ravel())))).reshape(T, D)
    else:
        dw = 1.0 if mutant == "delta_rows_by_one" else 0.5
        drop = {"stencil_neighbour_dropped_first": "first", "stencil_neighbour_dropped_last": "last"}.get(mutant)
        lik = omega * (_Wt(qt * E, D) - _Wt(qt * _W(y, D, dw=dw), D, drop=drop))
        lik_mag = omega * (_Wt(qt * np.abs(E), D, -1) + _Wt(qt * _W(np.abs(y), D, -1), D, -1)) if mags else None
    gv, gv_mag = gr.gv_term(p.pv, p.muv, y, mutant if mutant in GV_MUTANTS else None)
    return lik, gv, lik_mag, gv_mag


# ------------------------------------------------------------------------------------------------ the stencil
def _coefficients(p, mutant=None):
    """c0, c1, c2, r, r_mag, c2_mag (T,D) long double; c1_t / c2_t are the coefficients of y_{t-1} / y_{t-2} (zero where absent)"""
    T, D = p.T, p.D
    qt = p.q.astype(LD)[p.mhat - 1]
    ps, pd, pa = qt[:, :D], qt[:, D:2 * D], qt[:, 2 * D:]
    g, gm = qt * p.E.astype(LD), qt * p.Emag.astype(LD)
    c0 = ps + 4 * pa
    c0[1:] += pd[:-1] / 4 + pa[:-1]
    c0[:-1] += pd[1:] / 4 + pa[1:]
    if mutant == "boundary_diagonal_dropped":   # frames 1 and T-2 lose what the neighbour whose far side is absent adds
        c0[1] -= pd[0] / 4 + pa[0]
        c0[T - 2] -= pd[T - 1] / 4 + pa[T - 1]
    c1 = np.zeros((T, D), dtype=LD)
    c1[1:] = -2 * pa[:-1] - 2 * pa[1:]
    if mutant == "c1_wrong_neighbour":          # P[t,t+1] in the place of P[t-1,t] (p_a of frame T absent)
        c1[1:-1] = -2 * pa[1:-1] - 2 * pa[2:]
        c1[T - 1] = -2 * pa[T - 1]
    c2, c2m = np.zeros((T, D), dtype=LD), np.zeros((T, D), dtype=LD)
    c2[2:] = -pd[1:-1] / 4 + pa[1:-1]
    c2m[2:] = pd[1:-1] / 4 + pa[1:-1]
    if mutant == "c2_wrong_neighbour":          # from frame t+1 (absent for the last frame)
        c2[2:] = 0
        c2[2:T - 1] = -pd[3:] / 4 + pa[3:]
    if mutant == "c2_without_pa":               # the two-window coefficient
        c2[2:] = -pd[1:-1] / 4
    gs, gd, ga = g[:, :D], g[:, D:2 * D], g[:, 2 * D:]
    r = gs - 2 * ga
    r[1:] += gd[:-1] / 2 + ga[:-1]
    r[:-1] += -gd[1:] / 2 + ga[1:]
    if mutant == "r_delta_delta_dropped":
        r = gs.copy()
        r[1:] += gd[:-1] / 2
        r[:-1] -= gd[1:] / 2
    ms, md, ma = gm[:, :D], gm[:, D:2 * D], gm[:, 2 * D:]
    rmag = ms + 2 * ma
    rmag[1:] += md[:-1] / 2 + ma[:-1]
    rmag[:-1] += md[1:] / 2 + ma[1:]
    return c0, c1, c2, r, rmag, c2m


def _apply(c0, c1, c2, y):
    Py = c0 * y
    Py[1:] += c1[1:] * y[:-1]
    Py[:-1] += c1[1:] * y[1:]
    Py[2:] += c2[2:] * y[:-2]
    Py[:-2] += c2[2:] * y[2:]
    return Py


def stencil_terms(p, y, mutant=None):
    """(P y, r) (T,D) long double in the five-point form"""
    c0, c1, c2, r, _, _ = _coefficients(p, mutant)
    return _apply(c0, c1, c2, np.asarray(y, dtype=LD)), r


def lik_magnitude(p, y):
    """omega (W'|D^-1| Emag + |W|'|D^-1||W||y|) in the five-point form: gradient_terms' lik_mag with Emag for |E|"""
    c0, c1, _, _, rmag, c2m = _coefficients(p)
    return (rmag + _apply(c0, np.abs(c1), c2m, np.abs(np.asarray(y, dtype=LD)))) / (2 * p.T)


def gradient(p, y, mutant=None):
    """(lik, gv) (T,D) long double; the dense mutants through gradient_terms, the stencil's own here"""
    if mutant in DENSE_MUTANTS:
        lik, gv, _, _ = gradient_terms(p, y, mutant, mags=False)
        return lik, gv
    Py, r = stencil_terms(p, y, mutant if mutant != "gauss_seidel" else None)
    return (r - Py) / (2 * p.T), gr.gv_term(p.pv, p.muv, y)[0]


def step(p, y, alpha, mutant=None):
    """y + alpha (lik + gv)(y), long double.  gauss_seidel: frame t takes y_{t-1}, y_{t-2} from the new epoch, y_{t+1}, y_{t+2}
    from the old"""
    y = np.asarray(y, dtype=LD)
    if mutant != "gauss_seidel":
        lik, gv = gradient(p, y, mutant)
        return y + LD(alpha) * (lik + gv)
    c0, c1, c2, r, _, _ = _coefficients(p)
    gv = gr.gv_term(p.pv, p.muv, y)[0]
    new = y.copy()
    T = p.T
    for t in range(T):
        Py = c0[t] * y[t]
        if t >= 1:
            Py = Py + c1[t] * new[t - 1]
        if t + 1 < T:
            Py = Py + c1[t + 1] * y[t + 1]
        if t >= 2:
            Py = Py + c2[t] * new[t - 2]
        if t + 2 < T:
            Py = Py + c2[t + 2] * y[t + 2]
        new[t] = y[t] + LD(alpha) * ((r[t] - Py) / (2 * T) + gv[t])
    return new


def chain_length(p):
    """K of the step bar: gv_restatement.chain_length with 3 * 3D in the place of 3 * 2D (the docstring above)"""
    return 3 * 3 * p.D + p.T + p.D + gr.FMA_AND_TREE


def step_bar(p, alpha, y_n, y_n1, gv_mag):
    """gv_restatement.step_bar fed the five-point lik_magnitude (Emag for |E|), at the chain length above"""
    bar = gr.step_bar(p.D, p.T, alpha, y_n, y_n1, lik_magnitude(p, y_n), gv_mag)
    return bar * (LD(chain_length(p)) / gr.chain_length(p.D, p.T))


def ascent(p, y0, epochs, alpha, keep=(), fp64=False):
    """iterate step from y0; fp64: y is rounded to FP64 after every epoch (an FP64 ascent whose epochs are exact)"""
    y = np.asarray(y0, dtype=LD)
    kept = {}
    for n in range(epochs + 1):
        if n in keep:
            kept[n] = y.copy()
        if n < epochs:
            y = step(p, y, alpha)
            if fp64:
                y = y.astype(np.float64).astype(LD)
    return y, kept


def increment_bar(cond, rho, y, y_init, y_ml, inc, muv):
    """gv_restatement.increment_bar's form with the pentadiagonal system's condition number (the docstring above): bar on
    max |inc_a - inc_b| / max |inc|.  Every argument from the restatement's side: y, y_init, y_ml, inc (T,D)."""
    d = float(np.max(np.abs(np.asarray(y_init) - np.asarray(y_ml))))
    s = float(np.max(np.sqrt(np.asarray(muv) / np.asarray(y_ml).var(axis=0, ddof=1))))
    c = 64.0 * 2.0 * 2.0 * s * d / float(np.max(np.abs(inc)))
    return cond * rho * EPS * c / (d / float(np.max(np.abs(y))))


# ------------------------------------------------------------------------------------------------ the step-visible inputs
# The recipe of tests/gv_diag_restatement.py's cross-diagonal cases over three windows: model
# em_bdiag_restatement.bdiag_model(900 + D, 6D, M, sep = SEP); a PRESCRIBED mixture sequence (traj_full_restatement.sequence) and
# X_t = mu^x[s_t] + 0.3 sqrt(vx[s_t]) N(0, I) over the 3D source rows, which the arg-max takes with a clear margin (asserted on the
# host) -- the device and the restatement then work on the same mhat.  GV statistics: gv_restatement.gv_stats (asymmetric
# covariance) on the plain trajectory of the group's `cycle` utterance of STATS_T frames, the covariance times the case's
# cov_scale.  alpha and cov_scale per case: a grid search on the CPU (alpha in {1, 3} 10^k, scale in 10^k:
# tools/gv_penta_case_search.py) against gv_restatement's conditions -- both summands >= 0.2 of every checked step for n >= 1, the
# step >= 1e-5 of max |y|, y finite and within 10 max |y_0| -- never against the kernel.
SEP = 6.0
NOISE = 0.3
STATS_T = 50
N_FULL, N_SHORT = gr.N_FULL, gr.N_SHORT


class Case:
    def __init__(self, D, M, seq, T, alpha, cov_scale, ns=N_FULL):
        self.D, self.M, self.seq, self.T, self.alpha, self.cov_scale, self.ns = D, M, seq, T, alpha, cov_scale, ns

    @property
    def id(self):
        return f"D{self.D}-M{self.M}-T{self.T}"


def utterance(mdl, D, M, seq, T):
    """(X (T,3D), s 1-based)"""
    rng = np.random.default_rng([3, D, T])
    s = tf.sequence(seq, M, T, rng)
    _, mu, cov = mdl
    return mu[:3 * D, s].T + NOISE * np.sqrt(cov[:3 * D, s].T) * rng.standard_normal((T, 3 * D)), s + 1


@functools.lru_cache(maxsize=None)
def group(D, M):
    """(model, restatement converter, mu_v, Sigma_vv at scale 1) of a (D, M) group"""
    mdl = bdiag_model(900 + D, 6 * D, M, sep=SEP)
    conv = tp.PentaTrajectory(*mdl)
    Xs, s = utterance(mdl, D, M, "cycle", STATS_T)
    muv, Sv = gr.gv_stats(np.random.default_rng(D), conv.banded(Xs, s)[0])
    for a in (muv, Sv):
        a.setflags(write=False)
    return mdl, conv, muv, Sv


@functools.lru_cache(maxsize=None)
def _inputs(D, M, seq, T, cov_scale):
    mdl, conv, muv, Sv = group(D, M)
    X, s = utterance(mdl, D, M, seq, T)
    Sv = Sv * cov_scale
    p = pieces(conv, X, muv, Sv)
    y_ml, cond, rho = conv.banded(X, s)
    y0 = npo.variance_scaling(y_ml, muv)
    for a in (X, s, Sv, y0, y_ml):
        a.setflags(write=False)
    return dict(model=mdl, conv=conv, X=X, s=s, muv=muv, Sv=Sv, pieces=p, y0=y0, y_ml=y_ml, cond=cond, rho=rho)


def inputs(case):
    """model, restatement converter, X (T,3D), the prescribed sequence s (1-based), GV statistics, PentaPieces, the plain
    trajectory with its condition number and rho, and the eq. (58) start of a case -- made once, never written to"""
    return _inputs(case.D, case.M, case.seq, case.T, case.cov_scale)


# (D, M, seq, T, ns): D = 12 -- T = 2: no +-2 neighbour at all; 3, 4, 5: one, then both; 16, 17, 50: all boundary combinations
# inside a longer utterance; D = 33: 3D = 99 above bdmap_kernel's 96-row step, a row one past 32 lanes; D = 40: the ordinary
# shape, streamed (one array is 96 KB); D = 42: 3D = 126, the limit; M = 256: many mixtures; and at D = 12 the first and last T
# of every form of the launch rule: 269 / 270 (six arrays resident / five), 323 / 324, 403 / 404, 538 / 539 and 807 / 808 (two --
# the last T of an LDS-resident form -- / streamed); T = 2 is the first T of the six-array form
EDGE_TS = (269, 270, 323, 324, 403, 404, 538, 539, 807, 808)
SHAPES = ([(12, 4, "cycle", T, N_FULL) for T in (2, 3, 4, 5, 16, 17, 50)] +
          [(33, 3, "rand", 64, N_FULL), (33, 3, "rand", 65, N_FULL), (40, 8, "runs", 300, N_FULL), (42, 5, "cycle", 33, N_FULL),
           (4, 256, "cycle", 70, N_FULL)] +
          [(12, 4, "runs", T, N_SHORT) for T in EDGE_TS])
# one fvconvert_batch call across the launch rule: the batch runs streamed (its longest member), the members alone run with two
# and with five arrays resident
BATCH_TS = (808, 807, 270)

# (alpha, cov_scale) per (D, M, T), and for the batch: what tools/gv_penta_case_search.py prints
SETTINGS = {
    (12, 4, 2): (0.0003, 0.1), (12, 4, 3): (0.01, 1), (12, 4, 4): (0.0001, 0.01), (12, 4, 5): (0.01, 1), (12, 4, 16): (0.03, 1),
    (12, 4, 17): (0.03, 1), (12, 4, 50): (0.001, 0.01), (33, 3, 64): (0.03, 1), (33, 3, 65): (0.03, 1), (40, 8, 300): (0.3, 1),
    (42, 5, 33): (0.03, 1), (4, 256, 70): (0.003, 0.001), (12, 4, 269): (3, 10), (12, 4, 270): (3, 10), (12, 4, 323): (3, 10),
    (12, 4, 324): (3, 10), (12, 4, 403): (1, 1), (12, 4, 404): (3, 10), (12, 4, 538): (1, 1), (12, 4, 539): (1, 1),
    (12, 4, 807): (1, 1), (12, 4, 808): (0.003, 0.001),
}
BATCH_SETTING = (0.1, 0.1)


def _cases():
    return [Case(D, M, seq, T, *SETTINGS[(D, M, T)], ns) for D, M, seq, T, ns in SHAPES]


def _batch_cases():
    return [Case(12, 4, "runs", T, *BATCH_SETTING, N_SHORT) for T in BATCH_TS]


CASES = _cases()
BATCH_CASES = _batch_cases()
ALL_CASES = CASES + BATCH_CASES
