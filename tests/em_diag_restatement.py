"""Extended-precision (numpy longdouble) restatement of the diagonal-covariance M-step (test helper, not a test module), in
the style of tests/em_restatement.py: estep.py:mstep_diag / em_mstep_diag_kernel in longdouble, the generator of its cases and
element-wise error bounds of a float64 evaluation.  tests/test_em_diag_host.py proves the bounds against float64 numpy
before tests/test_gpu_em_diag.py judges the device by them.

Arrays are Julia-shaped: S0 (M,), S1, S2 (Dj,M); w (M,), mu, var (Dj,M)."""
import numpy as np

from em_restatement import EPS64, LD

# (Dj, M, mean scale): one thread of the kernel's workgroup per dimension up to its last (256), the strided total over M > 256,
# means large against the spread (the cancellation in S2 / S0 - mu^2)
MSTEP_DIAG_SHAPES = [(1, 1, 1.0), (2, 3, 1.0), (25, 5, 1e3), (80, 16, 1.0), (80, 128, 1.0), (160, 3, 1.0), (256, 2, 1e3),
                     (12, 257, 1.0), (8, 600, 10.0)]


def mstep_diag(S0, S1, S2, min_covar=1e-7):
    """estep.py:mstep_diag in longdouble, the same operations in the same order."""
    S0, S1, S2 = (np.asarray(a, dtype=LD) for a in (S0, S1, S2))
    w = S0 / (S0.sum() + 10 * EPS64) + EPS64
    inv = 1 / (S0 + 10 * EPS64)
    mu = S1 * inv[None, :]
    var = S2 * inv[None, :] - 2 * mu * S1 * inv[None, :] + mu * mu + LD(min_covar)
    return w, mu, var


def mstep_diag_case(seed, Dj, M, scale):
    """The diagonal analogue of em_restatement.mstep_case: S0 log-uniform in [1e-8, 1e6], means scale * N(0,1), variances the
    diagonal of A A' / Dj (A: Dj x (Dj+3)) -> S0 (M,), S1 = S0 mean, S2 = S0 (var + mean^2), float64."""
    rng = np.random.default_rng(seed)
    S0 = np.exp(rng.uniform(np.log(1e-8), np.log(1e6), M))
    S1 = np.empty((Dj, M))
    S2 = np.empty((Dj, M))
    for m in range(M):
        mean = scale * rng.standard_normal(Dj)
        A = rng.standard_normal((Dj, Dj + 3))
        S1[:, m] = S0[m] * mean
        S2[:, m] = S0[m] * (np.sum(A * A, axis=1) / Dj + mean * mean)
    return S0, S1, S2


def pack_diag_stats(S0, S1, S2, loglik):
    """Julia-shaped statistics -> the packed [S0 | S1 (Dj,M) | S2 (Dj,M) | loglik] buffer of vcmi_estep_stats_len doubles."""
    return np.concatenate([S0, np.asarray(S1).T.ravel(), np.asarray(S2).T.ravel(), [loglik]])


# Variances.  u = eps / 2 is the unit roundoff; starred quantities are exact.  First order in u:
#   inv  = fl(1 / fl(S0 + 10 eps))                       relative error 2u
#   mu   = fl(S1 inv)                                    3u
#   a    = fl(S2 inv)                                    3u        |da| <=  3u |S2| inv*
#   b    = fl(fl((2 mu) S1) inv),  b* = 2 mu*^2          3u + 2u + 2u = 7u   |db| <= 14u mu*^2      (2 mu is exact)
#   g    = fl(mu mu)                                     3u + 3u + u = 7u    |dg| <=  7u mu*^2
#   f    = fl(a - b)          adds  u |a - b|   <=  u (|S2| inv* + 2 mu*^2)
#   h    = fl(f + g)          adds  u |f + g|   <=  u (|S2| inv* + 3 mu*^2)
#   var  = fl(h + min_covar)  adds  u |var|     <=  u (|S2| inv* + 3 mu*^2 + min_covar)
# (the roundings of the variance's own expression -- four products, three additions, 2 mu exact -- on top of the inherited
# errors of inv and mu).  Sum:  (3 + 1 + 1 + 1) u |S2| inv* + (14 + 7 + 2 + 3 + 3) u mu*^2 + u min_covar
#   = 6u |S2| inv* + 29u mu*^2 + u min_covar  <=  10u (|S2| inv* + 3 mu*^2 + min_covar) = 5 eps (...).
# Contracting a product into the addition that consumes it (FMA) removes that product's rounding and adds none, so the count
# holds with or without contraction.  One more eps covers the second-order terms and the longdouble reference's own
# roundings (2^-64 each): the constant is 6.
VAR_BOUND_EPS = 6


def mstep_diag_bounds(S0, S1, S2, min_covar, ref):
    """Element-wise error bounds of a float64 diagonal M-step against ref = mstep_diag(...) in longdouble, from its operation
    count (eps = 2^-52): weights (12 + M/256) eps |w| (256 strided partial sums, an 8-level tree, the division and the
    addition -- as em_restatement.mstep_bounds); means 2 eps |mu| (sum, reciprocal, product: 3u); variances
    VAR_BOUND_EPS eps (|S2| inv + 3 mu^2 + min_covar), derived above."""
    w, mu, _ = ref
    M = len(S0)
    inv = 1 / (np.asarray(S0, dtype=LD) + 10 * EPS64)
    bw = (12 + M / 256.0) * EPS64 * np.abs(w)
    bmu = 2 * EPS64 * np.abs(mu)
    bvar = VAR_BOUND_EPS * EPS64 * (np.abs(np.asarray(S2, dtype=LD)) * inv[None, :] + 3 * mu * mu + LD(min_covar))
    return bw, bmu, bvar


def recovery_case(seed=31, N=20_000):
    """Frames of a 3-mixture, Dj = 4 diagonal model whose means are 20 standard deviations apart (along every axis the
    spacing is 20 times the largest standard deviation): X (N,Dj), the label of every frame, the true means (M,Dj) and
    standard deviations (M,Dj)."""
    rng = np.random.default_rng(seed)
    M, Dj = 3, 4
    sd = np.exp(rng.uniform(np.log(0.5), 0.0, (M, Dj)))            # in [0.5, 1]
    mu = 20.0 * np.arange(M)[:, None] * np.ones((1, Dj)) + rng.uniform(-1.0, 1.0, (M, Dj))
    lab = rng.choice(M, size=N, p=[0.5, 0.3, 0.2])
    X = mu[lab] + rng.standard_normal((N, Dj)) * sd[lab]
    return X, lab, mu, sd


def recovery_worst_deviation(X, lab, mu_true, mu_fit):
    """Fitted means (Dj,M) matched to the true mixtures (nearest true mean, which must be a bijection) -> the largest
    |fitted mean - sample mean of the mixture's own frames| in units of the standard error sqrt(var_d / N_m) of that
    sample mean (var_d: the sample variance of the same frames)."""
    M = len(mu_true)
    mu_fit = np.asarray(mu_fit, dtype=np.float64)
    match = [int(np.argmin(np.sum((mu_true - mu_fit[:, k]) ** 2, axis=1))) for k in range(M)]
    assert sorted(match) == list(range(M)), match
    worst = 0.0
    for k, m in enumerate(match):
        own = X[lab == m]
        se = np.sqrt(np.var(own, axis=0, ddof=1) / len(own))
        worst = max(worst, float(np.max(np.abs(mu_fit[:, k] - own.mean(axis=0)) / se)))
    return worst
