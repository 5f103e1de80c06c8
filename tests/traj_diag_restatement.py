"""numpy restatement of trajectory conversion with DIAGONAL conditional precisions (vcmi_traj_set_precision(t, DIAG),
csrc/traj_diag.hip) -- test infrastructure, in two forms that share only the model's arithmetic:

  sparse(X)    the reference's own statement with another precision matrix: oracle/np_oracle.py's TrajectoryGMMMap (explicit
               sparse W, block-diagonal D^-1, spsolve of W'D^-1W y = W'D^-1E) with Dy_m replaced by diag(q_m),
               q_m = 1 ./ diag(Sigma^yy_m - A_m Sigma^xy_m);
  tridiag(X)   what the device solves: per static dimension and frame parity one symmetric tridiagonal system
                   P[t,t] = p_s(t) + p_d(t-1)/4 + p_d(t+1)/4,  P[t,t-2] = -p_d(t-1)/4,  r[t] = g_s(t) + g_d(t-1)/2 - g_d(t+1)/2
               (terms with a frame outside the utterance dropped), [p_s ; p_d] = q[mhat_t], g_t = q[mhat_t] * E_t, each solved
               dense with numpy.linalg.solve; also returns the largest numpy.linalg.cond of those matrices -- the number the
               tolerances of the tests are derived from.

Arrays follow oracle/np_oracle.py: [frame, feature]."""
import numpy as np

from oracle import np_oracle as npo

EPS = 2.0 ** -53


def tolerance(cond):
    """relerr bound between two FP64 solutions of systems with this condition number: 64 cond 2^-53"""
    return 64.0 * cond * EPS


class DiagTrajectory:
    def __init__(self, w, mu, sig):
        self.g = npo.GMMMap(w, mu, sig)
        g = self.g
        self.C = np.stack([g.Syy[m] - g.A[m] @ g.Sxy[m] for m in range(g.M)])      # conditional covariances
        self.q = np.stack([1.0 / np.diag(self.C[m]) for m in range(g.M)])          # (M, 2D)
        self.tj = npo.TrajectoryGMMMap(g)
        self.tj.Dy = np.stack([np.diag(self.q[m]) for m in range(g.M)])

    def sparse(self, X):
        """X (T,2D) -> (T,D)"""
        if X.shape[0] == 0:
            return np.zeros((0, X.shape[1] // 2))
        return self.tj.fvconvert(X)[0]

    def tridiag(self, X):
        """X (T,2D) -> ((T,D), largest condition number of the tridiagonal matrices)"""
        g = self.g
        T, D2 = X.shape
        D = D2 // 2
        Y = np.zeros((T, D))
        if T == 0:
            return Y, 1.0
        mhat = g.predict(X)
        Ey = np.stack([g.muy[m - 1] + g.A[m - 1] @ (X[t] - g.mux[m - 1]) for t, m in enumerate(mhat)])
        p = self.q[mhat - 1]                       # (T, 2D)
        G = p * Ey
        ps, pd, gs, gd = p[:, :D], p[:, D:], G[:, :D], G[:, D:]
        diag = ps.copy()
        diag[1:] += 0.25 * pd[:-1]
        diag[:-1] += 0.25 * pd[1:]
        r = gs.copy()
        r[1:] += 0.5 * gd[:-1]
        r[:-1] -= 0.5 * gd[1:]
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
        return Y, cond

    def vc(self, fm, L):
        """vc(c, fm) of src/common.jl:31-63 with this model: fm (T, 2D+1) -> ((T, D+1), largest condition number); chunks of L"""
        T = fm.shape[0]
        D = (fm.shape[1] - 1) // 2
        out = np.empty((T, D + 1))
        cond = 1.0
        for b in range(0, T, L):
            y, c = self.tridiag(fm[b:b + L, 1:])
            out[b:b + L, 1:] = y
            cond = max(cond, c)
        out[:, 0] = fm[:, 0]
        return out, cond


def smooth_frames(rng, w, mu, sig, T, D):
    """the frames of tests/test_gpu_trajectory.py::test_vs_oracle_batch: a scaled cumulative sum of draws from the model, with
    its deltas; (T, 2D)"""
    static = npo.sample_frames(int(rng.integers(1 << 30)), w, mu, sig, T, 0, D)
    static = np.cumsum(static, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
    return npo.push_delta(static)


# (D, M, Ts): the shapes of the issue -- the headline dimension; the short utterances where the stencil loses neighbours; a
# dimension padded in the full path; one lane past a slab of 32 with both parities of T; 2D > 96
SHAPES = [(40, 8, [300]), (12, 4, [1, 2, 3, 4, 5, 50]), (7, 2, [30, 2]), (33, 3, [64, 65]), (59, 4, [33, 64])]


def make_case(D, M, Ts, seed_offset=500):
    """model and utterances as test_vs_oracle_batch makes them"""
    w, mu, sig = npo.synth_model(seed_offset + D, 4 * D, M, lam_lo=1e-3)
    rng = np.random.default_rng(D)
    return (w, mu, sig), [smooth_frames(rng, w, mu, sig, T, D) for T in Ts]


def diagonal_conditional_model(seed, D, M):
    """A joint model whose conditional covariance is diagonal by construction: Syx = A Sxx, Syy = diag(c) + A Sxx A'."""
    w, mu, sig = npo.synth_model(seed, 4 * D, M, lam_lo=1e-3)
    rng = np.random.default_rng(seed + 1)
    D2 = 2 * D
    out = np.empty_like(sig)
    for m in range(M):
        Sxx = sig[m][:D2, :D2]
        A = 0.3 * rng.standard_normal((D2, D2)) / np.sqrt(D2)
        c = np.exp(rng.uniform(np.log(1e-2), 0.0, D2))
        S = np.block([[Sxx, Sxx @ A.T], [A @ Sxx, np.diag(c) + A @ Sxx @ A.T]])
        out[m] = (S + S.T) / 2.0
    return w, mu, out


# variance scale of the delta rows and columns in the ill-conditioned model: p_d / p_s ~ 1 / ILL_SCALE^2
ILL_SCALE = 1.0e-4


def ill_conditioned_model(seed, D, M, scale=ILL_SCALE):
    """synth_model with the delta rows and columns of every Sigma scaled by `scale`: the delta precisions dominate the static
    ones by ~ scale^-2 and the tridiagonal matrices approach the singular second-difference operator"""
    w, mu, sig = npo.synth_model(seed, 4 * D, M, lam_lo=1e-3)
    s = np.ones(4 * D)
    s[D:2 * D] = scale
    s[3 * D:] = scale
    return w, mu * s, sig * s[None, :, None] * s[None, None, :]
