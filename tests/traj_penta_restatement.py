"""numpy restatement of trajectory conversion with THREE windows (static + delta + delta-delta) straight from a cross-diagonal
model (BlockDiagTrajectoryGMMMap(g, T, windows=3), vcmi_traj_create_bdiag_windows; the fused arg-max + g_t pass of
csrc/gmmmap_bdiag.hip over 3D rows and the pentadiagonal solver of csrc/traj_penta.hip) -- test infrastructure, written from the
cross-diagonal parameters alone.

Features are rows [static (D); delta (D); delta-delta (D)].  Per frame t, W has the static row (1 at t), the delta row (-1/2 at
t-1, +1/2 at t+1) and the delta-delta row (1 at t-1, -2 at t, 1 at t+1); entries whose frame lies outside the utterance are
dropped, the -2 is always there.  The log-densities, the first-maximum rule and
    a_km = c_km / vx_km,   q_km = 1 / (vy_km - a_km c_km) = [p_s ; p_d ; p_a],   g_kt = q_k,mhat (muy_k,mhat + a_k,mhat (x_kt - mux_k,mhat))
are those of tests/traj_bdiag_restatement.py over k = 0 .. 3D-1 (gmmmap_bdiag_restatement).  Y is then computed twice,
independently:

  dense(X)    from an explicit W: the conditional precisions are diagonal, so static dimensions decouple and W is the same
              (3T x T) matrix W1 for each of them; y_d = (W1' diag(p_d) W1) \\ (W1' g_d), numpy.linalg.solve on the products;
  banded(X)   from the closed form, per static dimension the symmetric pentadiagonal system
                  P[t,t]   = p_s(t) + p_d(t-1)/4 + p_d(t+1)/4 + p_a(t-1) + 4 p_a(t) + p_a(t+1)
                  P[t,t+1] = -2 p_a(t) - 2 p_a(t+1)                      (t+1 < T)
                  P[t,t+2] = -p_d(t+1)/4 + p_a(t+1)                      (t+2 < T)
                  r[t]     = g_s(t) + g_d(t-1)/2 - g_d(t+1)/2 + g_a(t-1) - 2 g_a(t) + g_a(t+1)
              (a p or g of a frame outside the utterance absent), assembled and solved densely; also returns the largest
              numpy.linalg.cond of those matrices and rho.

Tolerance of every comparison: relerr < traj_diag_restatement.tolerance(cond) * rho = 64 cond rho 2^-53.  The derivation is the
one in tests/traj_bdiag_restatement.py, with three more terms in the right-hand side.  Two FP64 evaluations of g agree
element-wise to a few eps of G = |q| (|muy| + |a dx|), not of |g| (muy and a dx may cancel).  r is a signed stencil over g, now
over six neighbours instead of three, so two right-hand sides differ by a few eps of
    r_abs[t] = G_s(t) + G_d(t-1)/2 + G_d(t+1)/2 + G_a(t-1) + 2 G_a(t) + G_a(t+1)          (every stencil sign taken positive)
-- the three delta-delta terms enter with the absolute values of their weights 1, 2, 1 -- and in the norm of the comparison by
a few eps rho ||r||, rho = ||r_abs||_inf / ||r||_inf >= 1.  The sum of six terms instead of three adds three roundings of at most
eps r_abs each, inside the same "few".  A system of condition number cond turns a relative perturbation delta of its right-hand
side into at most cond delta of the solution.  The solver is L D L' without pivoting, backward stable on symmetric positive
definite matrices (P = diag(p_s) + a Gram matrix, p_s > 0), so two solves of the same system differ by a modest multiple of
cond eps: run in plain FP64 the recurrence stayed at error / (64 cond 2^-53) <= 1.5e-2 against numpy.linalg.solve for T up to
2000 and precisions spread over five decades (tests/c/traj_penta_check.cpp repeats that against a long-double solve).  All of it
is inside 64 cond rho eps.

Arrays follow oracle/np_oracle.py: frames [frame, feature]; the model is Julia-shaped like tests/em_bdiag_restatement.py:
w (M,), mu (6D,M), covars (9D,M)."""
import numpy as np

import traj_bdiag_restatement as R2
from em_bdiag_restatement import bdiag_model, draw
from oracle import np_oracle as npo

# (D, M, Ts): a plain mid-size case over several frame tiles; the short utterances where the stencil loses one and two
# neighbours on each side; 3D = 21, padded rows in the tables; the limit 3D = 126 <= 128 on and one past a 64-frame tile; the
# limit on the shortest chains; the largest M (the pass's 32-frame tiles); the benchmark's model past two tiles
SHAPES = [(40, 8, [300]), (12, 4, [1, 2, 3, 4, 5, 50]), (7, 2, [30, 2]), (42, 3, [64, 65]), (42, 2, [1, 2, 3]), (4, 256, [70]),
          (40, 64, [130])]
# ... and the utterance of the vc test: T = 100 in chunks of 30
VC_CASE = (12, 4, [100])


def push_delta2(static):
    """static (T,D) -> (T,3D): [oracle push_delta | delta-delta], the delta-delta rows x_{t-1} - 2 x_t + x_{t+1} with absent
    neighbours dropped, summed left to right"""
    static = np.asarray(static, dtype=np.float64)
    a = -2.0 * static
    a[1:] = static[:-1] + a[1:]
    a[:-1] = a[:-1] + static[1:]
    return np.concatenate([npo.push_delta(static), a], axis=1)


def window_matrix(T):
    """W1 (3T,T) of ONE static dimension: rows 3t (static), 3t+1 (delta), 3t+2 (delta-delta)"""
    W = np.zeros((3 * T, T))
    for t in range(T):
        W[3 * t, t] = 1.0
        W[3 * t + 2, t] = -2.0
        if t >= 1:
            W[3 * t + 1, t - 1] = -0.5
            W[3 * t + 2, t - 1] = 1.0
        if t + 1 < T:
            W[3 * t + 1, t + 1] = 0.5
            W[3 * t + 2, t + 1] = 1.0
    return W


def construct_w(D, T):
    """dense (3DT, DT) W in the package's layout: row 3D t + block D + d, column D t + d"""
    W1 = window_matrix(T).reshape(T, 3, T)
    W = np.zeros((T, 3, D, T, D))
    for d in range(D):
        W[:, :, d, :, d] = W1
    return W.reshape(3 * D * T, D * T)


def make_case(D, M, Ts, swap=False):
    """model bdiag_model(900 + D, 6D, M); utterances: the source-static columns of draw(...) as a cumulative sum scaled by
    1/sqrt(t), with their deltas and delta-deltas; rng = default_rng(D)"""
    w, mu, cov = bdiag_model(900 + D, 6 * D, M)
    rng = np.random.default_rng(D)
    s0 = 3 * D if swap else 0
    Xs = []
    for T in Ts:
        static = draw(int(rng.integers(1 << 30)), w, mu, cov, T)[:, s0:s0 + D]
        static = np.cumsum(static, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
        Xs.append(push_delta2(static))
    return (w, mu, cov), Xs


class PentaTrajectory(R2.BdiagTrajectory):
    """mhat, undecided and g are BdiagTrajectory's (generic in the feature count, here 3D: self.D2 holds it)"""

    def __init__(self, w, mu, covars, swap=False):
        super().__init__(w, mu, covars, swap)
        self.D = self.D2 // 3

    def tridiag(self, X, mhat=None):
        raise NotImplementedError("three windows: banded / dense")

    def _parts(self, X, mhat):
        D = self.D
        _, p, G, Ga = self.g(X, mhat)
        cut = lambda a: (a[:, :D], a[:, D:2 * D], a[:, 2 * D:])          # noqa: E731
        return cut(p), cut(G), cut(Ga)

    def dense(self, X, mhat=None):
        """X (T,3D) -> (T,D) through the explicit window matrix"""
        T, D = X.shape[0], self.D
        if T == 0:
            return np.zeros((0, D))
        (ps, pd, pa), (gs, gd, ga), _ = self._parts(X, mhat)
        W1 = window_matrix(T)
        p = np.stack([ps, pd, pa], axis=1).reshape(3 * T, D)             # row 3t + block, as W1's rows
        g = np.stack([gs, gd, ga], axis=1).reshape(3 * T, D)
        P = np.stack([W1.T @ (p[:, d, None] * W1) for d in range(D)])    # (D,T,T) = W1' diag(p_d) W1
        r = W1.T @ g                                                      # (T,D)
        return np.linalg.solve(P, r.T[:, :, None])[:, :, 0].T

    def banded(self, X, mhat=None):
        """X (T,3D) -> ((T,D), largest condition number of the pentadiagonal matrices, rho)"""
        T, D = X.shape[0], self.D
        Y = np.zeros((T, D))
        if T == 0:
            return Y, 1.0, 1.0
        (ps, pd, pa), (gs, gd, ga), (As, Ad, Aa) = self._parts(X, mhat)
        diag = ps + 4.0 * pa
        diag[1:] += 0.25 * pd[:-1] + pa[:-1]
        diag[:-1] += 0.25 * pd[1:] + pa[1:]
        r = gs - 2.0 * ga
        r[1:] += 0.5 * gd[:-1] + ga[:-1]
        r[:-1] += -0.5 * gd[1:] + ga[1:]
        ra = As + 2.0 * Aa
        ra[1:] += 0.5 * Ad[:-1] + Aa[:-1]
        ra[:-1] += 0.5 * Ad[1:] + Aa[1:]
        P = np.zeros((D, T, T))
        k = np.arange(T)
        P[:, k, k] = diag.T
        if T > 1:
            e1 = (-2.0 * pa[:-1] - 2.0 * pa[1:]).T                       # (D,T-1): P[t,t+1]
            P[:, k[:-1], k[1:]] = e1
            P[:, k[1:], k[:-1]] = e1
        if T > 2:
            e2 = (-0.25 * pd[1:-1] + pa[1:-1]).T                         # (D,T-2): P[t,t+2] from frame t+1
            P[:, k[:-2], k[2:]] = e2
            P[:, k[2:], k[:-2]] = e2
        Y = np.linalg.solve(P, r.T[:, :, None])[:, :, 0].T
        cond = max(1.0, float(np.max(np.linalg.cond(P))))
        return Y, cond, float(np.max(ra) / np.max(np.abs(r)))

    def vc(self, fm, L):
        """vc(c, fm) of src/common.jl:31-63 with this model: fm (T, 3D+1) -> ((T, D+1), largest cond, largest rho); chunks of L"""
        T = fm.shape[0]
        out = np.empty((T, self.D + 1))
        cond = rho = 1.0
        for b in range(0, T, L):
            y, c, r = self.banded(fm[b:b + L, 1:])
            out[b:b + L, 1:] = y
            cond, rho = max(cond, c), max(rho, r)
        out[:, 0] = fm[:, 0]
        return out, cond, rho


def tie_case():
    """traj_bdiag_restatement.tie_case widened to three windows.  D = 3, M = 3, T = 10: mixtures 1 and 2 with bit-identical
    weights and source-side parameters and different target sides; mixture 3 with weight 0 and the frames' own mean"""
    D, M, T = 3, 3, 10
    (w, mu, cov), (X,) = make_case(D, M, [T])
    w, mu, cov = np.array([0.5, 0.5, 0.0]), mu.copy(), cov.copy()
    mu[:3 * D, 1] = mu[:3 * D, 0]
    cov[:3 * D, 1] = cov[:3 * D, 0]
    cov[6 * D:, 1] = 0.5 * cov[6 * D:, 0]              # another slope; the pair stays valid (|c| shrinks)
    mu[:3 * D, 2] = X.mean(axis=0)
    return (w, mu, cov), X
