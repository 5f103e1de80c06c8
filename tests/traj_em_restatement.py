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
"""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

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
