"""Extended-precision (numpy longdouble, 64-bit mantissa) restatement of the full-covariance EM blocks (test helper, not a
test module): Cholesky of Hermitian(Sigma), log-weighted densities by forward substitution, E-step statistics and the old
sklearn.mixture.GMM M-step with its guards, plus the generators of the ill-conditioned cases.  tests/test_em_host.py proves
it against 50-digit mpmath and against the float64 oracles before tests/test_gpu_em_blocks.py judges the device by it.

Arrays follow the oracle's convention: X (N,Dj); w (M,); mu (M,Dj); sigma (M,Dj,Dj) indexed [m][col][row] (the Julia
memory image), so Hermitian()'s upper triangle (row <= col, src/gmm.jl:16) is sigma[m][c][r] with r <= c.  chol() and
spd() work on one plain (row, col) matrix.  mstep_full takes and returns the Julia shapes of estep.py:mstep_full."""
import numpy as np

LD = np.longdouble
# no silent fall-back to float64: on a platform whose long double is a double the GPU tests that need this module skip
assert np.finfo(LD).eps < 1e-18, "numpy longdouble is not an extended-precision type on this platform"

PI = 4 * np.arctan(LD(1))
LOG2PI = np.log(2 * PI)
EPS64 = LD(np.finfo(np.float64).eps)


def chol(S):
    """Lower Cholesky factor of Hermitian(S) (upper triangle mirrored), column by column; LinAlgError on a pivot that is
    not > 0 (a NaN included)."""
    A = np.triu(np.asarray(S, dtype=LD))
    A = A + np.triu(A, 1).T
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j + 1} is not positive")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def logdens(X, w, mu, sigma):
    """(N,M) log w_m + log N(x_n; mu_m, Hermitian(Sigma_m)); z = L^-1 (x - mu) by forward substitution."""
    X = np.asarray(X, dtype=LD)
    N, Dj = X.shape
    M = len(w)
    out = np.empty((N, M), dtype=LD)
    for m in range(M):
        if not w[m] > 0:
            out[:, m] = -np.inf
            continue
        L = chol(np.asarray(sigma[m]).T)
        B = (X - np.asarray(mu[m], dtype=LD)).T                   # (Dj,N)
        Z = np.empty_like(B)
        for i in range(Dj):
            Z[i] = (B[i] - L[i, :i] @ Z[:i]) / L[i, i]
        logdet = 2 * np.sum(np.log(np.diag(L)))
        out[:, m] = np.log(LD(w[m])) - (Dj * LOG2PI + logdet) / 2 - np.sum(Z * Z, axis=0) / 2
    return out


def estep_full(X, w, mu, sigma):
    """S0 (M,), S1 (M,Dj), S2 (M,Dj,Dj), loglik -- softmax and sums in longdouble."""
    lpr = logdens(X, w, mu, sigma)
    Xl = np.asarray(X, dtype=LD)
    u = lpr.max(axis=1, keepdims=True)
    lse = u[:, 0] + np.log(np.sum(np.exp(lpr - u), axis=1))
    gam = np.exp(lpr - lse[:, None])
    S2 = np.stack([(Xl * gam[:, m, None]).T @ Xl for m in range(len(w))])
    return gam.sum(axis=0), gam.T @ Xl, S2, lse.sum()


def mstep_full(S0, S1, S2, min_covar=1e-7):
    """estep.py:mstep_full / em_mstep_full_kernel in longdouble: S0 (M,), S1 (Dj,M), S2 (Dj,Dj,M) -> w, mu (Dj,M),
    sigma (Dj,Dj,M)."""
    S0, S1, S2 = (np.asarray(a, dtype=LD) for a in (S0, S1, S2))
    Dj = S1.shape[0]
    w = S0 / (S0.sum() + 10 * EPS64) + EPS64
    inv = 1 / (S0 + 10 * EPS64)
    mu = S1 * inv[None, :]
    sigma = S2 * inv[None, None, :] - mu[:, None, :] * mu[None, :, :] + LD(min_covar) * np.eye(Dj, dtype=LD)[:, :, None]
    return w, mu, sigma


def spd(seed, Dj, cond):
    """Q diag(lam) Q' with lam log-spaced from 1 down to 1 / cond, exactly symmetrised (float64)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((Dj, Dj)))
    lam = np.logspace(0.0, -np.log10(cond), Dj) if Dj > 1 else np.ones(1)
    S = (Q * lam) @ Q.T
    return (S + S.T) / 2.0


def probe_frames(seed, mu, S, n, k=8):
    """-> (n frames drawn from N(mu, S), min(k, Dj) frames mu + 3 sqrt(lam_i) v_i along the eigen-directions of the k
    smallest eigenvalues of S): where the Mahalanobis term is most sensitive to an error of the factorisation."""
    rng = np.random.default_rng(seed)
    Dj = len(mu)
    lam, V = np.linalg.eigh(S)                                   # ascending
    drawn = mu + rng.standard_normal((n, Dj)) @ np.linalg.cholesky(S).T
    k = min(k, Dj)
    probes = mu + 3.0 * (np.sqrt(np.abs(lam[:k]))[:, None] * V[:, :k].T)
    return drawn, probes


# (Dj, M, mean scale): staging filled to its last slot (256), the strided total over M > 256, means large against the spread
MSTEP_SHAPES = [(1, 1, 1.0), (2, 3, 1.0), (25, 5, 1e3), (80, 16, 1.0), (99, 2, 30.0), (160, 3, 1.0), (255, 2, 1.0),
                (256, 2, 1e3), (12, 257, 1.0), (8, 600, 10.0)]


def mstep_case(seed, Dj, M, scale):
    """Host statistics of a model with S0 log-uniform in [1e-8, 1e6], means scale * N(0,1), Sigma = A A' / Dj
    (A: Dj x (Dj+3)): S0 (M,), S1 (Dj,M), S2 (Dj,Dj,M) -- float64, S2 exactly symmetric."""
    rng = np.random.default_rng(seed)
    S0 = np.exp(rng.uniform(np.log(1e-8), np.log(1e6), M))
    S1 = np.empty((Dj, M))
    S2 = np.empty((Dj, Dj, M))
    for m in range(M):
        mean = scale * rng.standard_normal(Dj)
        A = rng.standard_normal((Dj, Dj + 3))
        T = A @ A.T / Dj + np.outer(mean, mean)
        S1[:, m] = S0[m] * mean
        S2[:, :, m] = S0[m] * ((T + T.T) / 2.0)
    return S0, S1, S2


def pack_stats(S0, S1, S2, loglik):
    """Julia-shaped statistics -> the packed [S0 | S1 | S2 | loglik] buffer of vcmi_estep_full_stats_len doubles."""
    return np.concatenate([S0, S1.T.ravel(), np.transpose(S2, (2, 1, 0)).ravel(), [loglik]])


def mstep_bounds(S0, S1, S2, min_covar, ref):
    """Element-wise error bounds of a float64 M-step against ref = mstep_full(...) in longdouble, from its operation
    count (eps = 2^-52): weights (12 + M/256) eps |w| (256 strided partial sums, an 8-level tree, the division and the
    addition); means 2 eps |mu| (sum, reciprocal, product); covariances 4 eps (|S2| inv + |mu_r mu_c| + min_covar)
    (reciprocal, product, subtraction with or without FMA contraction, addition) -- scaled by the cancelled terms."""
    w, mu, _ = ref
    M = len(S0)
    inv = 1 / (np.asarray(S0, dtype=LD) + 10 * EPS64)
    bw = (12 + M / 256.0) * EPS64 * np.abs(w)
    bmu = 2 * EPS64 * np.abs(mu)
    bsig = 4 * EPS64 * (np.abs(np.asarray(S2, dtype=LD)) * inv[None, None, :] + np.abs(mu[:, None, :] * mu[None, :, :])
                        + LD(min_covar))
    return bw, bmu, bsig
