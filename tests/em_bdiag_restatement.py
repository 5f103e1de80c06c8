"""Restatement of the cross-diagonal ("block_diag") EM blocks (test helper, not a test module), in the style of
tests/em_diag_restatement.py: estep.py:mstep_bdiag / em_mstep_bdiag_kernel in numpy longdouble with element-wise error bounds of
a float64 evaluation, a CENTRED numpy E-step in float64 or longdouble (the log-density exactly as include/vcmi.h writes it), and
the generators of the cases.  tests/test_em_bdiag_host.py proves the bounds and the references on the host before
tests/test_gpu_em_bdiag.py judges the device by them.

Arrays are Julia-shaped: w (M,), mu (Dj,M), covars (Dj + D, M) = [var (Dj,M); c (D,M)], D = Dj / 2, pair d = rows (d, d + D);
S0 (M,), S1, S2 (Dj,M), Sxy (D,M).  Frames are X (N,Dj), as the oracles take them."""
import functools

import numpy as np

from em_diag_restatement import mstep_diag, mstep_diag_bounds
from em_restatement import EPS64, LD, LOG2PI

# (Dj, M, mean scale): one thread of the kernel's workgroup per pair up to its last (128), the strided total over M = 256,
# means large against the spread (the cancellation in S2 / S0 - mu^2 and in Sxy / S0 - mu_x mu_y)
MSTEP_BDIAG_SHAPES = [(2, 1, 1.0), (4, 3, 1.0), (26, 5, 1e3), (80, 16, 1.0), (80, 128, 1.0), (160, 3, 1.0), (256, 2, 1e3),
                      (12, 256, 1.0)]

# (Dj, M, N) of the E-step: the smallest; an odd number of pairs; neither pairs nor mixtures fill a tile of 16; the headline
# dimension; delta features; the two limits
ESTEP_BDIAG_SHAPES = [(2, 1, 1), (2, 3, 100), (6, 5, 1000), (34, 17, 3000), (80, 32, 20000), (160, 16, 4096), (256, 2, 500),
                      (8, 256, 2000)]
# ... and frame counts around the 64-frame workgroup and past a 1024-frame segment, at (16, 4)
ESTEP_BDIAG_NS = [63, 64, 65, 4097]


# ------------------------------------------------------------------------------------------------------- M-step
def mstep_bdiag(S0, S1, S2, Sxy, min_covar=1e-7):
    """estep.py:mstep_bdiag in longdouble, the same operations in the same order -> w (M,), mu (Dj,M), covars (Dj + D, M)."""
    w, mu, var = mstep_diag(S0, S1, S2, min_covar)
    D = mu.shape[0] // 2
    inv = 1 / (np.asarray(S0, dtype=LD) + 10 * EPS64)
    c = np.asarray(Sxy, dtype=LD) * inv[None, :] - mu[:D] * mu[D:]
    return w, mu, np.vstack([var, c])


def mstep_bdiag_case(seed, Dj, M, scale):
    """em_diag_restatement.mstep_diag_case with pairs: S0 log-uniform in [1e-8, 1e6], means scale * N(0,1), variances the
    diagonal of A A' / Dj, pair correlations uniform in (-0.9, 0.9) -> S0, S1 = S0 mean, S2 = S0 (var + mean^2),
    Sxy = S0 (c + mean_d mean_{d+D}), float64."""
    rng = np.random.default_rng(seed)
    D = Dj // 2
    S0 = np.exp(rng.uniform(np.log(1e-8), np.log(1e6), M))
    S1, S2, Sxy = np.empty((Dj, M)), np.empty((Dj, M)), np.empty((D, M))
    for m in range(M):
        mean = scale * rng.standard_normal(Dj)
        A = rng.standard_normal((Dj, Dj + 3))
        var = np.sum(A * A, axis=1) / Dj
        c = rng.uniform(-0.9, 0.9, D) * np.sqrt(var[:D] * var[D:])
        S1[:, m] = S0[m] * mean
        S2[:, m] = S0[m] * (var + mean * mean)
        Sxy[:, m] = S0[m] * (c + mean[:D] * mean[D:])
    return S0, S1, S2, Sxy


def pack_bdiag_stats(S0, S1, S2, Sxy, loglik):
    """Julia-shaped statistics -> the packed [S0 | S1 (Dj,M) | S2 (Dj,M) | Sxy (D,M) | loglik] buffer of
    vcmi_estep_bdiag_stats_len doubles, each (.,M) part mixture by mixture."""
    return np.concatenate([S0, np.asarray(S1).T.ravel(), np.asarray(S2).T.ravel(), np.asarray(Sxy).T.ravel(), [loglik]])


# Cross-covariances.  u = eps / 2, starred quantities exact, first order in u (the count of em_diag_restatement.py):
#   inv = fl(1 / fl(S0 + 10 eps))        relative error 2u
#   mu  = fl(S1 inv)                     3u
#   a   = fl(Sxy inv)                    3u                  |da| <= 3u |Sxy| inv*
#   g   = fl(mu_x mu_y)                  3u + 3u + u = 7u    |dg| <= 7u |mu_x* mu_y*|
#   c   = fl(a - g)             adds     u |a - g|  <=  u (|Sxy| inv* + |mu_x* mu_y*|)
# Sum: 4u |Sxy| inv* + 8u |mu_x* mu_y*|  <=  8u (|Sxy| inv* + |mu_x* mu_y*|) = 4 eps (...).  (Contraction into an FMA removes a
# rounding and adds none.)  One more eps covers the second-order terms and the longdouble reference's own roundings: 5.
C_BOUND_EPS = 5


def mstep_bdiag_bounds(S0, S1, S2, Sxy, min_covar, ref):
    """Element-wise error bounds of a float64 cross-diagonal M-step against ref = mstep_bdiag(...) in longdouble: weights, means
    and variances as em_diag_restatement.mstep_diag_bounds, cross-covariances C_BOUND_EPS eps (|Sxy| inv + |mu_d mu_{d+D}|),
    derived above.  -> bw (M,), bmu (Dj,M), bcov (Dj + D, M)"""
    w, mu, cov = ref
    Dj = mu.shape[0]
    D = Dj // 2
    bw, bmu, bvar = mstep_diag_bounds(S0, S1, S2, min_covar, (w, mu, cov[:Dj]))
    inv = 1 / (np.asarray(S0, dtype=LD) + 10 * EPS64)
    bc = C_BOUND_EPS * EPS64 * (np.abs(np.asarray(Sxy, dtype=LD)) * inv[None, :] + np.abs(mu[:D] * mu[D:]))
    return bw, bmu, np.vstack([bvar, bc])


def pairs_valid(covars):
    """(D,M) booleans: vx > 0, vy > 0, vx vy - c^2 > 0"""
    v = np.asarray(covars, dtype=LD)
    D = v.shape[0] // 3
    vx, vy, c = v[:D], v[D:2 * D], v[2 * D:]
    return (vx > 0) & (vy > 0) & (vx * vy - c * c > 0)


# ------------------------------------------------------------------------------------------------------- E-step
def estep_bdiag(X, w, mu, covars, dtype=np.float64):
    """The E-step of the cross-diagonal model in the centred form, one mixture at a time, in `dtype` (float64 or LD):
        det = vx vy - c^2,  l_nm = log w_m - (Dj log 2 pi + sum_d log det + sum_d (vy dx^2 - 2 c dx dy + vx dy^2) / det) / 2,
    responsibilities by a max-shifted softmax, S0 = sum gamma, S1 = gamma' z, S2 = gamma' z^2, Sxy = gamma' (z_d z_{d+D}),
    loglik = sum_n logsumexp_m l_nm.  -> S0 (M,), S1 (Dj,M), S2 (Dj,M), Sxy (D,M), loglik, all in `dtype`."""
    X, w, mu, cov = (np.asarray(a, dtype=dtype) for a in (X, w, mu, covars))
    N, Dj = X.shape
    D, M = Dj // 2, len(w)
    log2pi = LOG2PI if dtype is LD else dtype(float(LOG2PI))
    L = np.empty((N, M), dtype=dtype)
    for m in range(M):
        vx, vy, c = cov[:D, m], cov[D:Dj, m], cov[Dj:, m]
        det = vx * vy - c * c
        dx, dy = X[:, :D] - mu[:D, m], X[:, D:] - mu[D:, m]
        quad = ((vy * dx * dx - 2 * c * dx * dy + vx * dy * dy) / det).sum(axis=1)
        L[:, m] = np.log(w[m]) - (Dj * log2pi + np.log(det).sum() + quad) / 2
    u = L.max(axis=1)
    E = np.exp(L - u[:, None])
    s = E.sum(axis=1)
    G = E / s[:, None]
    Z = np.concatenate([X, X * X, X[:, :D] * X[:, D:]], axis=1)
    S = Z.T @ G                                                     # (2 Dj + D, M)
    return G.sum(axis=0), S[:Dj], S[Dj:2 * Dj], S[2 * Dj:], (u + np.log(s)).sum()


def bdiag_model(seed, Dj, M, sep=0.7, var_lo=0.05):
    """w (M,), mu (Dj,M), covars (Dj + D, M): per dimension a variance log-uniform in [var_lo, 1] and per pair a correlation
    uniform in (-0.9, 0.9), which every mixture varies (variances by exp(0.7 N(0,1) / sqrt(Dj)), correlations by
    0.3 N(0,1) / sqrt(D), kept inside (-0.9, 0.9)); means sep / sqrt(Dj) * N(0,1).  Everything that tells two mixtures apart
    is scaled by 1 / sqrt(Dj), so their distance over ALL dimensions together does not grow with Dj: the squared distance of
    two means is about 2 sep^2, divided by the variances (mean 1 / var about 3) and the pairs' 1 - rho^2 (mean of its inverse
    about 3) a Mahalanobis distance of about 3 -- a few standard deviations, so several mixtures share frames (the host test
    counts them)."""
    rng = np.random.default_rng(seed)
    D = Dj // 2
    w = rng.dirichlet(4.0 * np.ones(M))
    mu = np.asfortranarray(sep / np.sqrt(Dj) * rng.standard_normal((Dj, M)))
    var = np.exp(rng.uniform(np.log(var_lo), 0.0, (Dj, 1)) + 0.7 / np.sqrt(Dj) * rng.standard_normal((Dj, M)))
    rho = np.clip(rng.uniform(-0.9, 0.9, (D, 1)) + 0.3 / np.sqrt(D) * rng.standard_normal((D, M)), -0.9, 0.9)
    c = rho * np.sqrt(var[:D] * var[D:])
    return w, mu, np.asfortranarray(np.vstack([var, c]))


def draw(seed, w, mu, covars, N, labels=False):
    """(N,Dj) frames of the model: x = mu_x + sx z1, y = mu_y + sy (rho z1 + sqrt(1 - rho^2) z2)"""
    rng = np.random.default_rng(seed)
    Dj, M = mu.shape
    D = Dj // 2
    comp = rng.choice(M, size=N, p=np.asarray(w) / np.sum(w))
    sx, sy = np.sqrt(covars[:D]), np.sqrt(covars[D:Dj])
    rho = covars[Dj:] / (sx * sy)
    z1, z2 = rng.standard_normal((N, D)), rng.standard_normal((N, D))
    x = mu[:D].T[comp] + sx.T[comp] * z1
    y = mu[D:].T[comp] + sy.T[comp] * (rho.T[comp] * z1 + np.sqrt(1.0 - rho.T[comp] ** 2) * z2)
    X = np.concatenate([x, y], axis=1)
    return (X, comp) if labels else X


@functools.lru_cache(maxsize=None)
def estep_case(Dj, M, N):
    """model and frames of one E-step shape: made once, never written to"""
    w, mu, cov = bdiag_model(7000 + Dj + M, Dj, M)
    X = draw(7001 + N, w, mu, cov, N)
    for a in (w, mu, cov, X):
        a.setflags(write=False)
    return w, mu, cov, X


@functools.lru_cache(maxsize=None)
def estep_oracle(Dj, M, N):
    """the C oracle's full-covariance E-step on the expanded model of estep_case -> S0 (M,), S1 (Dj,M), S2 diag (Dj,M),
    Sxy (D,M), loglik: one of the two references the device is judged by; computed once per shape"""
    from oracle import c_oracle as co
    w, mu, cov, X = estep_case(Dj, M, N)
    return full_to_bdiag(*oracle_estep_full(co, X, w, mu, cov))


def expand(covars):
    """covars (Dj + D, M) -> (Dj,Dj,M), written independently of train.py:expand_block_diag (which the host test checks)"""
    cov = np.asarray(covars, dtype=np.float64)
    D, M = cov.shape[0] // 3, cov.shape[1]
    out = np.zeros((2 * D, 2 * D, M), order="F")
    for m in range(M):
        out[:, :, m] = np.diag(cov[:2 * D, m]) + np.diag(cov[2 * D:, m], D) + np.diag(cov[2 * D:, m], -D)
    return out


def oracle_estep_full(co, X, w, mu, covars):
    """co.estep_full on the expanded model, back in Julia shapes: S0 (M,), S1 (Dj,M), S2 (Dj,Dj,M), loglik"""
    sig = np.ascontiguousarray(np.transpose(expand(covars), (2, 1, 0)))
    S0, S1, S2, ll = co.estep_full(X, w, np.ascontiguousarray(np.asarray(mu).T), sig)
    return S0, S1.T, np.transpose(S2, (2, 1, 0)), ll


def full_to_bdiag(S0, S1, S2, ll):
    """full-covariance statistics S2 (Dj,Dj,M) -> the cross-diagonal ones: its (d,d) and (d,d+D) entries"""
    Dj = S2.shape[0]
    D = Dj // 2
    i, d = np.arange(Dj), np.arange(D)
    return S0, S1, S2[i, i, :], S2[d, d + D, :], ll


def cancellation_case(N=2000, Dj=8):
    """Two mixtures identical except for their weights (0.3, 0.7), so gamma is the known ratio for every frame: variances 1e-6,
    |mu| ~ 10, pair correlations +-(1 - 1e-6) alternating.  -> w, mu, covars, X (N,Dj)"""
    rng = np.random.default_rng(77)
    D = Dj // 2
    w = np.array([0.3, 0.7])
    m1 = 10.0 * np.where(rng.random(Dj) < 0.5, -1.0, 1.0) + 0.1 * rng.standard_normal(Dj)
    mu = np.asfortranarray(np.stack([m1, m1], axis=1))
    rho = (1.0 - 1e-6) * np.where(np.arange(D) % 2 == 0, 1.0, -1.0)
    col = np.concatenate([np.full(Dj, 1e-6), rho * 1e-6])
    cov = np.asfortranarray(np.stack([col, col], axis=1))
    return w, mu, cov, draw(78, w, mu, cov, N)


def recovery_case(seed=41, N=6000):
    """Frames of a 3-mixture, Dj = 4 cross-diagonal model whose means are 20 standard deviations apart along every axis, pair
    correlation 0.8 everywhere: X (N,Dj), the label of every frame."""
    rng = np.random.default_rng(seed)
    M, Dj = 3, 4
    var = np.exp(rng.uniform(np.log(0.25), 0.0, (Dj, M)))            # standard deviations in [0.5, 1]
    mu = 20.0 * np.arange(M)[None, :] * np.ones((Dj, 1)) + rng.uniform(-1.0, 1.0, (Dj, M))
    cov = np.vstack([var, 0.8 * np.sqrt(var[:2] * var[2:])])
    return draw(seed + 1, np.array([0.5, 0.3, 0.2]), mu, cov, N, labels=True)
