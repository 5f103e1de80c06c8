"""numpy restatement of the trajectory converter's EM re-estimation over all mixtures -- TEST INFRASTRUCTURE ONLY.

Toda, Black, Tokuda 2007, eqs. 30-36, in place of the suboptimum mixture sequence (their eq. 37) that
src/trajectory_gmmmap.jl:81-82 takes.  Written the way the reference is written -- explicit sparse W
(np_oracle.constructW), block-diagonal precision, spsolve -- and sharing no code with the product.

Notation (every array unsymmetrised, as np_oracle.TrajectoryGMMMap holds it):
    Q_m = Dy_m,  E_{m,t} = mu^y_m + A_m (X_t - mu^x_m),  pi_{m,t} = P(m | X_t)  (w_m <= 0 excluded),
    Y(y) = W y  (W's own boundary rule: a missing neighbour is dropped),  c_m = logdet((Q_m + Q_m')/2) / 2
E-step at y:   l_{m,t} = log pi_{m,t} + c_m - (Y_t - E_{m,t})' Q_m (Y_t - E_{m,t}) / 2 - D log 2 pi
               lse_t = logsumexp_m l_{m,t},  gamma_{m,t} = exp(l_{m,t} - lse_t),  L(y) = sum_t lse_t = log P(W y | X)
M-step:        Qbar_t = sum_m gamma_{m,t} Q_m,  gbar_t = sum_m gamma_{m,t} Q_m E_{m,t},
               (W' Qbar W) y = W' gbar
y^0 is np_oracle.TrajectoryGMMMap.fvconvert (arg-max of pi); iteration k maps y^k to y^{k+1}.

The module also holds the inputs of tests/test_gpu_traj_em.py (CASES, case_inputs), so that tests/test_traj_em_host.py can
check on the CPU that they are what the GPU assertions need, and one cache of the restatement's results.

Its second half (from "One pass term by term" on) serves tests/test_gpu_traj_em_terms.py and tests/test_traj_em_terms_host.py:
models whose pure and mixed frames lie side by side (HALF), frames on the pure / mixed decision line (LINE), one pass in
longdouble straight from (w, mu, Sigma) (estep_terms), its derived element-wise bounds and the flag band (estep_bounds), and
the checker both files apply (check_pass).
"""
import functools
import hashlib

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import gmmmap_restatement as GR
from em_restatement import LD, chol
from oracle import np_oracle as npo

LOG2PI = float(np.log(2.0 * np.pi))


class Model:
    """The per-model constants of the statement above."""

    def __init__(self, w, mu, sig):
        self.g = npo.GMMMap(w, mu, sig)
        self.tj = npo.TrajectoryGMMMap(self.g)
        self.Q = self.tj.Dy                                                   # (M, 2D, 2D), unsymmetrised
        self.c = np.array([0.5 * np.linalg.slogdet(0.5 * (q + q.T))[1] for q in self.Q])
        for q in self.Q:
            np.linalg.cholesky(0.5 * (q + q.T))                               # the objective needs it positive definite

    def log_prior(self, X):
        """log pi (T, M); -inf for a zero weight"""
        lw = np.stack([self.g.log_weighted(x) for x in X])
        u = lw.max(axis=1, keepdims=True)
        return lw - (u + np.log(np.sum(np.exp(lw - u), axis=1, keepdims=True)))

    def means(self, X):
        """E (M, T, 2D)"""
        g = self.g
        return np.stack([g.muy[m] + (X - g.mux[m]) @ g.A[m].T for m in range(g.M)])

    def estep(self, X, y, logpi=None, E=None):
        """y (T, D) -> l (M, T), lse (T), gamma (M, T), L"""
        T, D2 = X.shape
        D = D2 // 2
        logpi = self.log_prior(X) if logpi is None else logpi
        E = self.means(X) if E is None else E
        Y = (npo.constructW(D, T) @ y.ravel()).reshape(T, D2)
        e = Y[None] - E
        q = np.einsum("mti,mij,mtj->mt", e, self.Q, e)
        ell = logpi.T + self.c[:, None] - 0.5 * q - D * LOG2PI
        u = ell.max(axis=0)
        lse = u + np.log(np.sum(np.exp(ell - u), axis=0))
        return ell, lse, np.exp(ell - lse), float(np.sum(lse))


def em_convert(w, mu, sig, X, n):
    """X (T, 2D) -> dict: ys [n+1] of (T, D); L [n+1]; gamma [n+1] of (M, T); gap [n+1] of (T): l of the best mixture minus l of
    the second best (inf with one live mixture).  Entry k belongs to y^k."""
    mdl = Model(w, mu, sig)
    T, D2 = X.shape
    D = D2 // 2
    W = npo.constructW(D, T)
    logpi, E = mdl.log_prior(X), mdl.means(X)
    y = mdl.tj.fvconvert(X)[0]
    out = {"ys": [], "L": [], "gamma": [], "gap": []}
    for k in range(n + 1):
        ell, lse, gamma, L = mdl.estep(X, y, logpi, E)
        top = np.sort(ell, axis=0)
        out["ys"].append(y)
        out["L"].append(L)
        out["gamma"].append(gamma)
        out["gap"].append(top[-1] - top[-2] if len(top) > 1 else np.full(T, np.inf))
        if k == n:
            break
        Qbar = np.einsum("mt,mij->tij", gamma, mdl.Q)
        gbar = np.einsum("mt,mij,mtj->ti", gamma, mdl.Q, E)
        Dinv = sp.block_diag([sp.csc_matrix(q) for q in Qbar], format="csc")
        P = (W.T @ Dinv @ W).tocsc()
        y = spla.spsolve(P, W.T @ gbar.ravel()).reshape(T, D)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# inputs of the GPU tests.  name -> (kind, D, M, Ts, synth_model arguments, scale of the means, index of a zeroed weight)
# overlapping: every frame of the longer utterances is a blend in every iteration; peaked: no frame is
NITER = 4
CASES = {
    "stencil-12": ("overlap", 12, 4, (1, 2, 3, 4, 5, 17, 50), dict(lam_lo=0.5), 0.02, None),
    "native-16": ("overlap", 16, 4, (40, 3), dict(lam_lo=0.5), 0.02, None),
    "native-20": ("overlap", 20, 6, (64, 7, 0, 33), dict(lam_lo=0.5), 0.02, None),
    "padded-13": ("overlap", 13, 3, (33, 1), dict(lam_lo=0.5), 0.02, None),
    "padded-7": ("overlap", 7, 2, (30, 2), dict(lam_lo=0.5), 0.02, None),
    "cfg5-40": ("overlap", 40, 8, (48,), dict(lam_lo=0.5), 0.01, None),
    "big-48": ("overlap", 48, 3, (20,), dict(lam_lo=0.5), 0.01, None),
    "valu-52": ("overlap", 52, 3, (20,), dict(lam_lo=0.5), 0.01, None),          # 2D = 104 > 96: the per-frame E-step by itself
    "valu-66": ("overlap", 66, 2, (12, 3), dict(lam_lo=0.5), 0.01, None),        # ... with the solver's window in HBM (D > 64)
    "valu-130": ("overlap", 130, 2, (6,), dict(lam_lo=0.9), 0.001, None),        # 2D = 260 > 256: two rows per thread
    "zero-weight-12": ("overlap", 12, 4, (50, 9), dict(lam_lo=0.5), 0.02, 2),
    "peaked-12": ("peaked", 12, 4, (50, 5, 1), dict(lam_lo=1e-3), 1.0, None),
    "peaked-20": ("peaked", 20, 6, (64, 7), dict(lam_lo=1e-3), 1.0, None),
    "peaked-13": ("peaked", 13, 3, (33,), dict(lam_lo=1e-3), 1.0, None),
}
OVERLAP = [k for k, v in CASES.items() if v[0] == "overlap"]
PEAKED = [k for k, v in CASES.items() if v[0] == "peaked"]


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> (w, mu, sig), [X (T, 2D) per utterance]; frames as tests/test_gpu_trajectory.py::test_vs_oracle_batch builds them"""
    kind, D, M, Ts, kw, scale, zero = CASES[name]
    w, mu, sig = npo.synth_model((900 if kind == "overlap" else 500) + D, 4 * D, M, **kw)
    mu = mu * scale
    if zero is not None:
        w = w.copy()
        w[zero] = 0.0
        w /= w.sum()
    rng = np.random.default_rng(D)
    Xs = []
    for T in Ts:
        if T == 0:
            Xs.append(np.zeros((0, 2 * D)))
            continue
        static = npo.sample_frames(int(rng.integers(1 << 30)), w, mu, sig, T, 0, D)
        static = np.cumsum(static, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
        Xs.append(npo.push_delta(static))
    return (w, mu, sig), Xs


@functools.lru_cache(maxsize=None)
def case_reference(name, n=NITER):
    """the restatement's result for every non-empty utterance of the case (None for an empty one), computed once"""
    (w, mu, sig), Xs = case_inputs(name)
    return [em_convert(w, mu, sig, X, n) if len(X) else None for X in Xs]


@functools.lru_cache(maxsize=None)
def fixture_reference(n=NITER):
    """the reference's trained model (static 20 + delta 20) on trajectory_fixture_model.npz's X"""
    from conftest import load_golden
    z = load_golden("model_clb_to_slt_gmm32_order40_diff.npz")
    X = load_golden("trajectory_fixture_model.npz")["X"]
    return (z["weights"], z["means"], z["covars"]), X, em_convert(z["weights"], z["means"], z["covars"], X, n)


# ======================================================================================================================
# One pass term by term (tests/test_traj_em_terms_host.py, tests/test_gpu_traj_em_terms.py; the bounds are derived in
# DESIGN 3.4-EM "one pass term by term" and restated in estep_bounds' docstring)
EPS = 2.0 ** -53
TINY = 2.0 ** -1022                                                    # below it an FP64 exponential has no relative accuracy
SECOND = 1.0 + 2.0 ** -20                                              # the second-order terms of every first-order bound


def hg(n):
    """Higham's gamma_n = n eps / (1 - n eps): n chained roundings"""
    return n * EPS / (1.0 - n * EPS)


# name -> (D, overlapping mixtures Mo, isolated mixtures Mi, Ts, isolated frames per 16-frame tile, special)
#   edge: frames 1023 and 1024 of the first utterance (the scan's chunk edge) carry an overlapping label
#   late: the last isolated mixture is the label of frames t >= 64 only (the first workgroup skips it through need[])
#   gap:  frames 64 .. 127 all carry overlapping labels (the second workgroup skips the whole isolated group)
HALF = {
    "half-12": (12, 3, 3, (1100, 200, 65, 64, 63, 17, 1), 8, "edge"),
    "half-12-m33": (12, 30, 3, (130,), 8, None),                       # M odd and above 32: nine k-steps in the blend
    "half-13": (13, 3, 3, (130,), 8, None),                            # solved in 16 dimensions: Qpad
    "half-20": (20, 4, 4, (130,), 8, "late"),
    "half-40": (40, 5, 3, (130,), 13, "gap"),
    "half-48": (48, 2, 2, (80,), 8, None),
    "half-52": (52, 2, 1, (70,), 8, None),                             # 2D = 104 > 96: the per-frame kernel, fallback solver
}


@functools.lru_cache(maxsize=None)
def half_inputs(name):
    """-> (w, mu, sig), [X (T, 2D)], [labels z (T)]: overlapping mixtures 0 .. Mo-1 (the model of the "overlap" cases), isolated
    mixtures Mo + k whose source means are moved by 6 (k + 1) in every coordinate; frame t is drawn from the source marginal of
    mixture z_t.  Never written to."""
    D, Mo, Mi, Ts, per_tile, special = HALF[name]
    w, mu, sig = npo.synth_model(900 + D, 4 * D, Mo + Mi, lam_lo=0.5)
    mu = mu * 0.02
    rng = np.random.default_rng(7000 + 10 * D + Mo)
    for k in range(Mi):
        mu[Mo + k, :2 * D] += 6.0 * (k + 1) * rng.choice([-1.0, 1.0], size=2 * D)
    Ls = [np.linalg.cholesky(sig[m][:2 * D, :2 * D]) for m in range(Mo + Mi)]
    Xs, Zs = [], []
    for T in Ts:
        z = np.empty(T, dtype=np.int64)
        for t0 in range(0, T, 16):
            n = min(16, T - t0)
            free = np.array([i for i in range(n) if not (special == "edge" and T > 1024 and t0 + i in (1023, 1024))])
            npure = 0 if (special == "gap" and 64 <= t0 < 128) else (per_tile * n) // 16
            lab = rng.integers(0, Mo, n)
            pick = rng.choice(free, size=npure, replace=False)
            lab[pick] = Mo + rng.integers(0, Mi - (1 if special == "late" and t0 < 64 else 0), npure)
            z[t0:t0 + n] = lab
        Z = rng.standard_normal((T, 2 * D))
        Xs.append(np.stack([mu[m, :2 * D] + Ls[m] @ zz for m, zz in zip(z, Z)]))
        Zs.append(z)
    return (w, mu, sig), Xs, Zs


@functools.lru_cache(maxsize=None)
def half_reference(name, n=NITER):
    (w, mu, sig), Xs, _ = half_inputs(name)
    return [em_convert(w, mu, sig, X, n) for X in Xs]


def inverse_ld(S):
    """inv(S) of a general matrix in longdouble: Gauss-Jordan with partial pivoting"""
    n = S.shape[0]
    a = np.concatenate([np.asarray(S, dtype=LD), np.eye(n, dtype=LD)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        if p != c:
            a[[c, p]] = a[[p, c]]
        a[c] = a[c] / a[c, c]
        f = a[:, c].copy()
        f[c] = 0
        a -= f[:, None] * a[c][None, :]
    return a[:, n:]


class TermModel:
    """The constants of the statement at the top in longdouble, straight from (w, mu, Sigma), and the element-wise bounds on
    what the library's host preparation (csrc/traj_prepare.cpp, csrc/gmmmap_prepare.cpp: FP64) makes of them."""

    def __init__(self, w, mu, sig):
        w, mu = np.asarray(w, dtype=np.float64), np.asarray(mu, dtype=np.float64)
        assert np.all(w > 0.0)
        self.src = GR.Model(w, mu, sig)                                # the source side: log w_m N(x; mux_m, Sxx_m), A_m
        self.M, K = mu.shape[0], mu.shape[1] // 2
        self.K, self.D = K, K // 2
        S = np.transpose(np.asarray(sig, dtype=np.float64), (0, 2, 1))
        self.A, self.Q, self.b, self.c, self.dA, self.dQ, self.db, self.dc = ([] for _ in range(8))
        self.cond = 1.0
        for m in range(self.M):
            A, G = self.src.slope(m)
            Sxy, Syy = S[m, :K, K:], S[m, K:, K:]
            C = Syy.astype(LD) - A @ Sxy.astype(LD)
            Q = inverse_ld(C)
            L = chol(0.5 * (Q + Q.T))
            mux, muy = self.src.mux[m], self.src.muy[m]
            self.A.append(A)
            self.Q.append(Q)
            self.b.append(muy - A @ mux)
            self.c.append(np.log(np.diag(L)).sum())
            # --- the preparation's rounding (estep_bounds (0))
            Aa, Qa, Ca = (np.abs(a).astype(np.float64) for a in (A, Q, C))
            dA = (2 * K + 16) * EPS * G
            dC = (K + 2) * EPS * (np.abs(Syy) + Aa @ np.abs(Sxy)) + dA @ np.abs(Sxy)
            dQ = Qa @ dC @ Qa + (2 * K + 1) * EPS * (Qa @ Ca @ Qa)
            L64 = L.astype(np.float64)
            Ku = np.abs(np.linalg.inv(L64)) @ np.abs(L64)
            self.dA.append(dA)
            self.dQ.append(dQ)
            self.db.append((K + 2) * EPS * (np.abs(muy).astype(np.float64) + Aa @ np.abs(mux).astype(np.float64)) + dA @ np.abs(mux).astype(np.float64))
            self.dc.append(0.5 * float((Ca * dQ.T).sum()) + 0.5 * (K + 1) * EPS * float((Ku * Ku).sum())
                           + (K + 2) * EPS * float(np.abs(np.log(np.diag(L64))).sum())
                           + 3 * EPS * (abs(float(self.c[-1])) + self.D * LOG2PI))
            self.cond = max(self.cond, float(np.linalg.cond(S[m])))


def model_key(model):
    """a (w, mu, sig) triple by its contents: a copy of a model is the same model"""
    h = hashlib.sha256()
    for a in model:
        a = np.ascontiguousarray(a, dtype=np.float64)
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def _models_of(key):
    return {}


def term_model(model):
    """one TermModel per model (by contents)"""
    slot = _models_of(model_key(model))
    if "term" not in slot:
        slot["term"] = TermModel(*model)
    return slot["term"]


def float_model(model):
    """one float64 Model per model (by contents)"""
    slot = _models_of(model_key(model))
    if "float" not in slot:
        slot["float"] = Model(*model)
    return slot["float"]


def stencil(y, dtype=LD, wrap=False, weight=0.5):
    """y (T, D) -> Y (T, 2D) = W y.  (wrap / weight: the mutants of tests/test_traj_em_terms_host.py)"""
    y = np.asarray(y, dtype=dtype)
    Y = np.zeros((y.shape[0], 2 * y.shape[1]), dtype=dtype)
    D = y.shape[1]
    Y[:, :D] = y
    Y[:-1, D:] += weight * y[1:]
    Y[1:, D:] -= weight * y[:-1]
    if wrap:
        Y[-1, D:] += weight * y[-1]
        Y[0, D:] -= weight * y[0]
    return Y


def estep_terms(model, X, y):
    """One pass at y in longdouble -> dict: lp (T,M) log pi; E (M,T,K); Y, (e, v) per mixture; q, ell (T,M); lse (T); gamma (T,M);
    gbar (T,K); Qbar (T,K,K); best (T); r (T) = sum_{m != best} exp(l_m - l_best)"""
    tm = term_model(model)
    X = np.asarray(X, dtype=LD)
    T, M, K = X.shape[0], tm.M, tm.K
    Ls = tm.src.logdens(np.asarray(X, dtype=np.float64))
    us = Ls.max(axis=1)
    lsx = us + np.log(np.exp(Ls - us[:, None]).sum(axis=1))
    lp = Ls - lsx[:, None]
    Y = stencil(y)
    E = np.stack([tm.b[m] + X @ tm.A[m].T for m in range(M)])
    e = Y[None] - E
    v = np.stack([e[m] @ tm.Q[m].T for m in range(M)])
    q = (e * v).sum(axis=2).T
    cm = np.array([c - tm.D * GR.LOG2PI for c in tm.c], dtype=LD)
    ell = lp + cm[None, :] - q / 2
    best = np.argmax(ell, axis=1)
    u = ell[np.arange(T), best]
    ex = np.exp(ell - u[:, None])
    ex_other = ex.copy()
    ex_other[np.arange(T), best] = 0
    r = ex_other.sum(axis=1)
    lse = u + np.log1p(r)
    gamma = np.exp(ell - lse[:, None])
    vE = np.stack([E[m] @ tm.Q[m].T for m in range(M)])                # Q_m E_mt (M,T,K)
    gbar = np.einsum("tm,mtk->tk", gamma, vE)
    Qbar = np.einsum("tm,mij->tij", gamma, np.stack(tm.Q))
    return dict(lp=lp, Ls=Ls, lsx=lsx, E=E, Y=Y, e=e, v=v, vE=vE, q=q, cm=cm, ell=ell, lse=lse, gamma=gamma, gbar=gbar, Qbar=Qbar,
                best=best, r=r)


def estep_bounds(model, X, y):
    """Element-wise bounds on one pass of csrc/traj_em.hip at y around estep_terms (eps = 2^-53, gamma_n = n eps / (1 - n eps),
    K = 2D, starred = longdouble; every bound is a function of the inputs and of the longdouble evaluation, none of a result
    under test; first order, times 1 + 2^-20).

     (0) the host preparation in FP64, element-wise (gmmmap_restatement's statement for A; the cond 2^-53 term: |Q| |C| |Q| is
         cond(C) |Q| in size, and cond <= 2 for the models used -- asserted by the host test):
           dA = (2K + 16) eps |Syx| |inv Sxx| (I + |Sxx| |inv Sxx|)                 (Gauss-Jordan inverse, K-term products)
           dC = (K + 2) eps (|Syy| + |A| |Sxy|) + dA |Sxy|,   C = Syy - A Sxy
           dQ = |Q| dC |Q| + (2K + 1) eps |Q| |C| |Q|                               (the inverse of the rounded C, and its own rounding)
           db = (K + 2) eps (|muy| + |A| |mux|) + dA |mux|
           dc = 1/2 sum |C| o dQ' + 1/2 (K + 1) eps | |inv L| |L| |_F^2 + (K + 2) eps sum |log L_ii| + 3 eps (|c| + D log 2 pi)
                (d logdet Q = tr(inv(Q) dQ); Cholesky of the symmetrised Q: Higham 10.3; K logarithms and additions)
     (1) l_mt.  Y's delta rows carry one rounding: dY = eps (|y_{t+1}| + |y_{t-1}|) / 2.  e = Y - b - A x is one subtraction and
         a 2D-term MFMA chain (or as many fmas): de = gamma_{K+2} (|Y| + |b| + |A| |x|) + dY + db + dA |x|.  v = Q e, another:
         dv = gamma_K |Q| |e| + |Q| de + dQ |e|.  q = e . v: four fmas per lane, two lane exchanges, up to six waves (per-frame
         kernel: ceil(K / 256) fmas and an eight-level tree) -- at most 16: dq = gamma_16 |e|.|v| + de.|v| + |e|.dv + de.dv.
         log pi = ls - lse_m ls: Bpi = Bs_mt + max_m Bs_mt + (M + 16) eps (1 + |lse_m ls|), Bs = gmmmap_restatement.logdens_bound.
           B_mt = Bpi + dc_m + dq / 2 + 3 eps (|log pi| + |c_m - D log 2 pi| + q / 2)
     (2) lse_t:  BL_t = log1p(sum_m gamma*_mt expm1(B_mt)) + (M + 16) eps (1 + |lse_t|)       (tests/traj_em_bdiag_restatement.py (2))
     (3) gamma_mt, relative G_mt = expm1(B_mt + BL_t + 2 eps |l - lse| + (M + 16) eps):  dgamma = gamma* G + 2^-1022 (an FP64
         exponential below the normal range is flushed or keeps no relative accuracy: the mixtures need[] skips).
         With h_m = |b_m| + |A_m| |x|:
           |d gbar_t| <= sum_m dgamma |Q_m| h_m + sum_m gamma* (gamma_{2K+M+4} |Q_m| h_m + |Q_m| (db_m + dA_m |x|) + dQ_m h_m)
           |d Qbar_t| <= sum_m dgamma |Q_m| + sum_m gamma* (gamma_{M+4} |Q_m| + dQ_m)
         (E = b + A x: K + 1 roundings; Q E: K; the M-term weighted sums: M + 1 for gbar, M + 4 for the blend's k-loop, which
         is padded to a multiple of four.)

    THE FLAG BAND.  The kernel calls a frame pure when its COMPUTED 1 - exp(mx - (mx + log s)) is below 2^-53, s = 1 + r~ the sum
    of the exponentials, r~ within e^{+-2 B_t} of r = sum_{m != best} exp(l_m - l_best), B_t = max_m B_mt.
      pure for certain:  r~ < 2^-53 rounds s to 1, so lse = mx and the difference is 0.  With the M roundings of the sum and
        margin: r <= 2^-56 e^{-2 B_t}, flag = best.
      mixed for certain: log s >= r~ (1 - r~ / 2) - 2^-53 - M eps r~ (s rounds by half an ulp of 1); lse = fl(mx + log s) moves
        by at most half an ulp of mx, <= 2^-53 |mx|, and is absorbed altogether below that; d = mx - lse is exact; exp(d) and
        1 - exp(d) round by 2^-53 each and 1 - exp(d) >= |d| - d^2 / 2.  So the computed difference is at least
        r~ - (|mx| + 4) 2^-53 - O(r~^2), and it reaches 2^-53 from r~ = (|mx| + 5) 2^-53 <= 6 max(1, |mx|) 2^-53 on.  With margin
        for |mx| against |l_best| and the second order: r >= 8 max(1, |l_best|) 2^-53 e^{2 B_t}.
      between the two either answer is accepted, consistently (check_pass), and a pure frame's operands may differ from the exact
      blend by the bounds above plus what one-hot weights drop: r_t (|Q_best| + max_m |Q_m|), r_t (|Q E|_best + max_m |Q_m E_m|).

    -> dict of float64 arrays: ell (T,M), lse (T), gamma (T,M), gbar (T,K), Qbar (T,K,K), gslack (T,K), Qslack (T,K,K),
       must_mix (T), must_pure (T), Bt (T), and the longdouble terms `ref`"""
    tm = term_model(model)
    ref = estep_terms(model, X, y)
    X64 = np.asarray(X, dtype=np.float64)
    xa = np.abs(X64)
    T, M, K, D = X64.shape[0], tm.M, tm.K, tm.D
    f64 = lambda a: np.abs(np.asarray(a, dtype=np.float64))                            # noqa: E731
    Bs = tm.src.logdens_bound(X64)
    Bpi = Bs + Bs.max(axis=1, keepdims=True) + ((M + 16) * EPS * (1 + f64(ref["lsx"])))[:, None]
    ya = np.abs(np.asarray(y, dtype=np.float64))
    dY = np.zeros((T, K))
    dY[:-1, D:] += 0.5 * EPS * ya[1:]
    dY[1:, D:] += 0.5 * EPS * ya[:-1]
    Ya = f64(ref["Y"])
    B = np.empty((T, M))
    hq, dEq, dQh = [], [], []
    for m in range(M):
        Aa, Qa, ba = f64(tm.A[m]), f64(tm.Q[m]), f64(tm.b[m])
        hm = ba + xa @ Aa.T
        dEm = tm.db[m] + xa @ tm.dA[m].T
        de = hg(K + 2) * (Ya + hm) + dY + dEm
        ea, va = f64(ref["e"][m]), f64(ref["v"][m])
        dv = hg(K) * (ea @ Qa.T) + de @ Qa.T + ea @ tm.dQ[m].T
        dq = hg(16) * (ea * va).sum(axis=1) + (de * va).sum(axis=1) + (ea * dv).sum(axis=1) + (de * dv).sum(axis=1)
        B[:, m] = SECOND * (Bpi[:, m] + tm.dc[m] + 0.5 * dq + 3 * EPS * (f64(ref["lp"][:, m]) + abs(float(ref["cm"][m])) + 0.5 * f64(ref["q"][:, m])))
        hq.append(hm @ Qa.T)
        dEq.append(dEm @ Qa.T)
        dQh.append(hm @ tm.dQ[m].T)
    gam = f64(ref["gamma"])
    BL = SECOND * (np.log1p((gam * np.expm1(B)).sum(axis=1)) + (M + 16) * EPS * (1 + f64(ref["lse"])))
    dist = f64(ref["ell"] - ref["lse"][:, None])
    dgam = SECOND * gam * np.expm1(B + BL[:, None] + 2 * EPS * dist + (M + 16) * EPS) + TINY
    gb, Qb = np.zeros((T, K)), np.zeros((T, K, K))
    Qmax, vEmax = np.zeros((K, K)), np.zeros((T, K))
    for m in range(M):
        Qa = f64(tm.Q[m])
        gb += dgam[:, m:m + 1] * hq[m] + gam[:, m:m + 1] * (hg(2 * K + M + 4) * hq[m] + dEq[m] + dQh[m])
        Qb += dgam[:, m, None, None] * Qa[None] + gam[:, m, None, None] * (hg(M + 4) * Qa + tm.dQ[m])[None]
        Qmax = np.maximum(Qmax, Qa)
        vEmax = np.maximum(vEmax, f64(ref["vE"][m]))
    best = ref["best"]
    r = np.asarray(ref["r"], dtype=np.float64)
    Qbest = np.stack([f64(tm.Q[m]) for m in range(M)])[best]
    vEbest = f64(ref["vE"])[best, np.arange(T)]
    Bt = B.max(axis=1)
    lbest = f64(ref["ell"])[np.arange(T), best]
    return dict(ell=B, lse=BL, gamma=dgam, gbar=SECOND * gb, Qbar=SECOND * Qb, gslack=r[:, None] * (vEbest + vEmax),
                Qslack=r[:, None, None] * (Qbest + Qmax[None]), must_mix=r >= 8 * np.maximum(1.0, lbest) * EPS * np.exp(2 * Bt),
                must_pure=r <= 2.0 ** -56 * np.exp(-2 * Bt), Bt=Bt, ref=ref, tm=tm)


def check_pass(b, out):
    """What tests/test_gpu_traj_em_terms.py asserts of one pass `out` = dict(gamma (T,M), lse (T), flag (T), gbar (T,K), mh (T),
    count, table (count,K,K)) against estep_bounds' `b` -> (ratios: largest error / bound per term, problems: list of strings; a
    pass is right when every ratio is finite and <= 1 and there is no problem: accepted()).  A value that is not finite is a
    problem by itself: a NaN compares false with everything, so no ratio may be trusted to catch it."""
    ref = b["ref"]
    T, M = ref["gamma"].shape
    f64 = lambda a: np.asarray(a, dtype=np.float64)                                    # noqa: E731
    flag, mh, gamma = np.asarray(out["flag"]), np.asarray(out["mh"]), np.asarray(out["gamma"])
    problems = []
    mixed = flag == -1
    pure = ~mixed
    if np.any((flag < -1) | (flag >= M)):
        problems.append(f"flag outside -1 .. M-1 at frames {np.flatnonzero((flag < -1) | (flag >= M))[:8]}")
        flag = np.clip(flag, -1, M - 1)
    if np.any(pure & b["must_mix"]):
        problems.append(f"frames {np.flatnonzero(pure & b['must_mix'])[:8]} are flagged pure inside the mixed region")
    if np.any(mixed & b["must_pure"]):
        problems.append(f"frames {np.flatnonzero(mixed & b['must_pure'])[:8]} are flagged mixed inside the pure region")
    if np.any(pure & (flag != ref["best"])):
        problems.append(f"pure frames {np.flatnonzero(pure & (flag != ref['best']))[:8]} do not take the best mixture")
    onehot = np.zeros((T, M))
    onehot[np.arange(T), np.maximum(flag, 0)] = 1.0
    if np.any(gamma[pure] != onehot[pure]):
        problems.append("gamma of a pure frame is not exactly one-hot at its flag")
    if int(out["count"]) != int(mixed.sum()):
        problems.append(f"count {out['count']} but {int(mixed.sum())} frames are flagged mixed")
    want_mh = np.where(mixed, M + np.cumsum(mixed), flag + 1)         # M + k + 1, k = the frame's rank among the mixed, in frame order
    if np.any(mh != want_mh):
        problems.append(f"mh differs from the flags at frames {np.flatnonzero(mh != want_mh)[:8]}")
    for key in ("lse", "gamma", "gbar", "table"):
        if not np.all(np.isfinite(out[key])):
            problems.append(f"{key} holds {int((~np.isfinite(out[key])).sum())} values that are not finite")
    ratios = {}
    ratios["lse"] = float(np.max(np.abs(out["lse"] - f64(ref["lse"])) / b["lse"]))
    ratios["gamma"] = float(np.max((np.abs(gamma - f64(ref["gamma"])) / b["gamma"])[mixed], initial=0.0))
    ratios["gbar"] = float(np.max(np.abs(out["gbar"] - f64(ref["gbar"])) / (b["gbar"] + pure[:, None] * b["gslack"])))
    # the precision the solver reads for frame t: table entry mh - 1, the model's own matrix or a blended one
    Qs = np.stack([f64(q) for q in b["tm"].Q])
    k = np.clip(mh - M - 1, 0, max(len(out["table"]) - 1, 0))
    own = (mh >= 1) & (mh <= M)
    P = np.where(own[:, None, None], Qs[np.clip(mh - 1, 0, M - 1)], out["table"][k] if len(out["table"]) else 0.0)
    if np.any((mh < 1) | (mh > M + len(out["table"]))):
        problems.append("mh points outside the table")
    ratios["Qbar"] = float(np.max(np.abs(P - f64(ref["Qbar"])) / (b["Qbar"] + pure[:, None, None] * b["Qslack"])))
    return ratios, problems


def accepted(ratios, problems):
    """the verdict on check_pass' result (a NaN ratio is a rejection: `nan <= 1` is false, but max() may step over it)"""
    return not problems and all(np.isfinite(v) and v <= 1.0 for v in ratios.values())


NAN_MUTANTS = ("nan-lse", "nan-gamma", "nan-gbar", "nan-table")        # one NaN in one result (float_pass)
MUTANTS = ("wrap", "weight", "no-c", "unnormalised", "swap-gamma", "shift-workgroup", "drop-small", "blend-k+1", "pure-m+1")


def float_pass(model, X, y, mutant=None):
    """One pass in float64 numpy in the shape of the test hook's results (the kernel's decision rule, statement by statement)
    -- what check_pass is tried on without a device; mutant: one of MUTANTS or NAN_MUTANTS, a pass that is wrong in one place"""
    w, mu, sig = model
    mdl = float_model(model)
    X = np.asarray(X, dtype=np.float64)
    T, K = X.shape
    M = mdl.g.M
    if mutant == "unnormalised":
        logpi = np.stack([mdl.g.log_weighted(x) for x in X])
    else:
        logpi = mdl.log_prior(X)
    E = mdl.means(X)
    Y = stencil(y, np.float64, wrap=mutant == "wrap", weight=1.0 if mutant == "weight" else 0.5)
    e = Y[None] - E
    q = np.einsum("mti,mij,mtj->tm", e, mdl.Q, e)
    c = np.zeros(M) if mutant == "no-c" else mdl.c
    ell = logpi + c[None, :] - 0.5 * q - (K // 2) * LOG2PI
    if mutant == "shift-workgroup" and T > 65:
        ell[64:-1] = ell[65:].copy()
    mi = np.argmax(ell, axis=1)
    mx = ell[np.arange(T), mi]
    lse = mx + np.log(np.exp(ell - mx[:, None]).sum(axis=1))
    pure = 1.0 - np.exp(mx - lse) < 2.0 ** -53
    gamma = np.exp(ell - lse[:, None])
    gamma[pure] = 0.0
    gamma[pure, mi[pure]] = 1.0
    if mutant == "swap-gamma":
        t = int(np.flatnonzero(pure[:-1] != pure[1:])[0]) if np.any(pure[:-1] != pure[1:]) else 0
        gamma[[t, t + 1]] = gamma[[t + 1, t]]
    flag = np.where(pure, mi, -1).astype(np.int32)
    gg = np.where(gamma < 1e-8, 0.0, gamma) if mutant == "drop-small" else gamma
    gbar = np.einsum("tm,mij,mtj->ti", gg, mdl.Q, E)
    mixed = ~pure
    mh = np.where(mixed, M + np.cumsum(mixed), mi + (2 if mutant == "pure-m+1" else 1)).astype(np.int64)
    table = np.einsum("tm,mij->tij", gamma[mixed], mdl.Q)
    if mutant == "blend-k+1":
        table = np.roll(table, 1, axis=0)
    if mutant == "nan-lse":
        lse[T // 2] = np.nan
    if mutant == "nan-gamma":
        gamma[np.flatnonzero(mixed)[-1], M - 1] = np.nan
    if mutant == "nan-gbar":
        gbar[T // 3, K - 1] = np.nan
    if mutant == "nan-table":
        table[len(table) // 2, 1, 2] = np.nan
    return dict(gamma=gamma, lse=lse, flag=flag, gbar=gbar, mh=mh, count=int(mixed.sum()), table=table, ell=ell)


# ---- frames on the pure / mixed decision line -------------------------------------------------------------------------
LINE_LEVELS = (-30.0, -36.0, -36.5, -36.7468, -36.7368, -36.7268, -37.0, -37.5, -40.0, -45.0)     # log r_t of the target frames
LINE = {"line-64": 64, "line-130": 130}                               # the model and the frame recipe of "stencil-12", T frames
LINE_CLEAR = (-42.0, -26.0)                                           # no neighbour of a target has its log r in here


@functools.lru_cache(maxsize=None)
def line_inputs(name):
    """-> (w, mu, sig), X (T, 2D), y (T, D), levels (T; nan for a frame that is no target).  An all-overlap model; y is the
    arg-max solution with every fourth frame (t = 1, 5, ...) moved along a seeded random direction, by bisection on the
    longdouble evaluation, until log r_t is the frame's level.  y_t enters frame t through its static rows alone and its
    neighbours are not moved, so the targets do not interact.  Moving y_t does move the delta rows of frames t -+ 1 (and of no
    other target's neighbours): a direction that leaves log r of either inside LINE_CLEAR -- near the undecided band, where
    only targets are meant to be -- is passed over for the next of the seeded sequence."""
    T, D, M = LINE[name], 12, 4
    w, mu, sig = npo.synth_model(900 + D, 4 * D, M, lam_lo=0.5)
    mu = mu * 0.02
    rng = np.random.default_rng(100 + T)
    static = npo.sample_frames(int(rng.integers(1 << 30)), w, mu, sig, T, 0, D)
    static = np.cumsum(static, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
    X = npo.push_delta(static)
    model = (w, mu, sig)
    y = Model(*model).tj.fvconvert(X)[0].copy()
    tm = term_model(model)
    base = estep_terms(model, X, y)
    levels = np.full(T, np.nan)

    def logr(s, yc):
        """log r of frame s with the trajectory yc"""
        Ys = np.zeros(2 * D, dtype=LD)
        Ys[:D] = yc[s]
        if s + 1 < T:
            Ys[D:] += np.asarray(yc[s + 1], dtype=LD) / 2
        if s >= 1:
            Ys[D:] -= np.asarray(yc[s - 1], dtype=LD) / 2
        e = Ys[None] - base["E"][:, s]
        ell = np.array([base["lp"][s, m] + base["cm"][m] - (e[m] @ tm.Q[m] @ e[m]) / 2 for m in range(M)], dtype=LD)
        return float(np.log(np.sort(np.exp(ell - ell.max()))[:-1].sum()))

    for i, t in enumerate(range(1, T, 4)):
        lev = LINE_LEVELS[i % len(LINE_LEVELS)]
        y0 = y[t].copy()
        for attempt in range(64):
            d = rng.standard_normal(D)
            d /= np.linalg.norm(d)

            def at(a):
                y[t] = y0 + a * d
                return logr(t, y)

            lo, hi = 0.0, 1.0
            while at(hi) > lev:
                lo, hi = hi, 2.0 * hi
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                if at(mid) > lev:
                    lo = mid
                else:
                    hi = mid
            y[t] = y0 + hi * d
            if all(not LINE_CLEAR[0] < logr(s, y) < LINE_CLEAR[1] for s in (t - 1, t + 1) if s < T):
                break
        else:
            raise AssertionError(f"{name}: no direction for frame {t}")
        levels[t] = lev
    y.setflags(write=False)
    return model, X, y, levels
