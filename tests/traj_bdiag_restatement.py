"""numpy restatement of trajectory conversion straight from a CROSS-DIAGONAL model (BlockDiagTrajectoryGMMMap,
vcmi_traj_create_bdiag; the fused arg-max + g_t pass of csrc/gmmmap_bdiag.hip and the solver of csrc/traj_diag.hip) -- test
infrastructure, written from the cross-diagonal parameters alone: no (4D,4D,M) tensor, no inverse.

Per mixture m and feature k = 0 .. 2D-1, source side x and target side y after the swap:
    l_tm  = log w_m - (2D log 2 pi + sum_k log vx_km + sum_k (x_kt - mux_km)^2 / vx_km) / 2     (gmmmap_bdiag_restatement.logdens)
    mhat_t = first maximum of l_tm over m, 1-based
    a_km  = c_km / vx_km,   q_km = 1 / (vy_km - a_km c_km) = [p_s ; p_d]
    g_kt  = q_k,mhat (muy_k,mhat + a_k,mhat (x_kt - mux_k,mhat))
then, per static dimension and frame parity, the tridiagonal systems of tests/traj_diag_restatement.py
    P[t,t] = p_s(t) + p_d(t-1)/4 + p_d(t+1)/4,  P[t,t-2] = -p_d(t-1)/4,  r[t] = g_s(t) + g_d(t-1)/2 - g_d(t+1)/2
assembled and solved densely, with the largest numpy.linalg.cond of those matrices.

Tolerance of every comparison: relerr < traj_diag_restatement.tolerance(cond) * rho = 64 cond rho 2^-53.  Derivation.  Two FP64
evaluations of g agree element-wise to a few eps of |q| (|muy| + |a dx|), not of |g|: the centred form has no b_m vector, so
muy and a dx may cancel in g, and an evaluation that contracts them into one fma, or forms A x + b first as the dense path does,
differs by that much.  r is a signed stencil over g, so two right-hand sides differ by a few eps of
    r_abs[t] = G_s(t) + G_d(t-1)/2 + G_d(t+1)/2,   G = |q| (|muy| + |a dx|)          (every stencil sign taken positive)
and in the norm of the comparison by a few eps rho ||r||, rho = ||r_abs||_inf / ||r||_inf >= 1.  A system of condition number
cond turns a relative perturbation delta of its right-hand side into at most cond delta of the solution, and two backward-stable
solves of the same system differ by a modest multiple of cond eps themselves.  Both are inside 64 cond rho eps: the 64 of
traj_diag_restatement.tolerance is the solvers' margin, and since rho >= 1 the few eps of g (at most 6: the difference, the
quotient a, the product or fma, q with its own three roundings) are inside it too.

Arrays follow oracle/np_oracle.py: frames [frame, feature]; the model is Julia-shaped like tests/em_bdiag_restatement.py:
w (M,), mu (4D,M), covars (6D,M)."""
import numpy as np

import gmmmap_bdiag_restatement as BR
from em_bdiag_restatement import bdiag_model, draw
from oracle import np_oracle as npo

# (D, M, Ts): the headline dimension; the short utterances where the stencil loses neighbours; an odd dimension below a slab of
# 32; one lane past a slab with both parities of T; the largest dimension (2D = 128) with T off and on the 64-frame tile; the
# largest M (M = 256 does not fit LDS beside a 64-frame tile: the kernel's 32-frame tiles); the headline M past two tiles
SHAPES = [(40, 8, [300]), (12, 4, [1, 2, 3, 4, 5, 50]), (7, 2, [30, 2]), (33, 3, [64, 65]), (64, 5, [33, 64]), (4, 256, [70]),
          (40, 64, [130])]
# ... and the utterance of the vc tests: T = 100 in chunks of 30
VC_CASE = (12, 4, [100])


def make_case(D, M, Ts, swap=False):
    """model bdiag_model(900 + D, 4D, M); utterances: the source-static columns of draw(...) as a cumulative sum scaled by
    1/sqrt(t), with their deltas; rng = default_rng(D)"""
    w, mu, cov = bdiag_model(900 + D, 4 * D, M)
    rng = np.random.default_rng(D)
    s0 = 2 * D if swap else 0
    Xs = []
    for T in Ts:
        static = draw(int(rng.integers(1 << 30)), w, mu, cov, T)[:, s0:s0 + D]
        static = np.cumsum(static, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
        Xs.append(npo.push_delta(static))
    return (w, mu, cov), Xs


class BdiagTrajectory:
    def __init__(self, w, mu, covars, swap=False):
        self.model = (np.asarray(w, dtype=np.float64), np.asarray(mu, dtype=np.float64), np.asarray(covars, dtype=np.float64))
        self.swap = swap
        cov = self.model[2]
        D2 = cov.shape[0] // 3
        self.D2, self.D, self.M = D2, D2 // 2, cov.shape[1]
        _, self.mux, self.muy, vx, self.a = BR.split(*self.model, swap)
        vy, c = (cov[:D2] if swap else cov[D2:2 * D2]), cov[2 * D2:]
        self.q = 1.0 / (vy - self.a * c)                   # (2D, M)

    def mhat(self, X):
        """1-based first maximum of the centred log-density"""
        return BR.predict(BR.logdens(X, *self.model, self.swap))

    def undecided(self, X):
        """-> (top-two log-density gap per frame, 2 max_m B_tm per frame): a frame whose gap is not above the bound is one whose
        arg-max two correct FP64 evaluations may settle differently"""
        L = np.sort(BR.logdens(X, *self.model, self.swap), axis=1)
        gap = L[:, -1] - L[:, -2] if L.shape[1] > 1 else np.full(X.shape[0], np.inf)
        B = BR.logdens_bound(X, *self.model, self.swap)
        return gap, 2.0 * np.where(np.isfinite(B), B, 0.0).max(axis=1)

    def g(self, X, mhat=None):
        """-> (mhat (T,), p = q[mhat] (T,2D), g (T,2D), G = |q| (|muy| + |a dx|) (T,2D))"""
        m = (self.mhat(X) if mhat is None else np.asarray(mhat)) - 1
        mux, muy, a, p = self.mux.T[m], self.muy.T[m], self.a.T[m], self.q.T[m]
        adx = a * (X - mux)
        return m + 1, p, p * (muy + adx), np.abs(p) * (np.abs(muy) + np.abs(adx))

    def tridiag(self, X, mhat=None):
        """X (T,2D) -> ((T,D), largest condition number of the tridiagonal matrices, rho)"""
        T, D = X.shape[0], self.D
        Y = np.zeros((T, D))
        if T == 0:
            return Y, 1.0, 1.0
        _, p, G, Ga = self.g(X, mhat)
        ps, pd, gs, gd = p[:, :D], p[:, D:], G[:, :D], G[:, D:]
        diag = ps.copy()
        diag[1:] += 0.25 * pd[:-1]
        diag[:-1] += 0.25 * pd[1:]
        r, ra = gs.copy(), Ga[:, :D].copy()
        r[1:] += 0.5 * gd[:-1]
        r[:-1] -= 0.5 * gd[1:]
        ra[1:] += 0.5 * Ga[:-1, D:]
        ra[:-1] += 0.5 * Ga[1:, D:]
        cond = 1.0
        for par in (0, 1):
            fr = np.arange(par, T, 2)
            K = len(fr)
            if K == 0:
                continue
            P = np.zeros((D, K, K))
            k = np.arange(K)
            P[:, k, k] = diag[fr].T
            if K > 1:
                e = -0.25 * pd[fr[1:] - 1].T       # (D, K-1): P[t,t-2] = -p_d(t-1)/4
                P[:, k[1:], k[:-1]] = e
                P[:, k[:-1], k[1:]] = e
            Y[fr] = np.linalg.solve(P, r[fr].T[:, :, None])[:, :, 0].T
            cond = max(cond, float(np.max(np.linalg.cond(P))))
        return Y, cond, float(np.max(ra) / np.max(np.abs(r)))

    def vc(self, fm, L):
        """vc(c, fm) of src/common.jl:31-63 with this model: fm (T, 2D+1) -> ((T, D+1), largest cond, largest rho); chunks of L"""
        T = fm.shape[0]
        out = np.empty((T, self.D + 1))
        cond = rho = 1.0
        for b in range(0, T, L):
            y, c, r = self.tridiag(fm[b:b + L, 1:])
            out[b:b + L, 1:] = y
            cond, rho = max(cond, c), max(rho, r)
        out[:, 0] = fm[:, 0]
        return out, cond, rho


def expanded_model(w, mu, covars):
    """the dense model in oracle/np_oracle.py's shapes: w (M,), mu (M,4D), sig (M,4D,4D); em_bdiag_restatement.expand"""
    from em_bdiag_restatement import expand
    return np.asarray(w), np.ascontiguousarray(np.asarray(mu).T), np.ascontiguousarray(np.transpose(expand(covars), (2, 1, 0)))


def tie_case():
    """D = 3, M = 3, T = 10: mixtures 1 and 2 with bit-identical weights and source-side parameters and different target sides;
    mixture 3 with weight 0 and the frames' own mean (it would win on density alone)"""
    D, M, T = 3, 3, 10
    (w, mu, cov), (X,) = make_case(D, M, [T])
    w, mu, cov = np.array([0.5, 0.5, 0.0]), mu.copy(), cov.copy()
    mu[:2 * D, 1] = mu[:2 * D, 0]
    cov[:2 * D, 1] = cov[:2 * D, 0]
    cov[4 * D:, 1] = 0.5 * cov[4 * D:, 0]              # another slope; the pair stays valid (|c| shrinks)
    mu[:2 * D, 2] = X.mean(axis=0)
    return (w, mu, cov), X
