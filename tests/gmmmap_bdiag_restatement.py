"""Restatement of frame-by-frame conversion with a cross-diagonal ("block_diag") joint GMM (test helper, not a test module):
BlockDiagGMMMap / csrc/gmmmap_bdiag.hip in numpy, float64 or longdouble, CENTRED form, independent of train.py and of the
library; and the error bounds tests/test_gpu_gmmmap_bdiag.py holds the device to.  tests/test_gmmmap_bdiag_host.py checks this
file against oracle/np_oracle.GMMMap on the expanded model before the device is judged by it.

Arrays are Julia-shaped: w (M,), mu (Dj,M), covars (Dj + D, M) = [var (Dj,M); c (D,M)], D = Dj / 2.  Frames are X (T,D), results
Y (T,D), P (T,M), L (T,M), as the oracles take and give them.

The model, source side x and target side y (swap exchanges the halves; c is unchanged):
    l_tm = log w_m - (D log 2 pi + sum_d log vx_dm + sum_d (x_dt - mux_dm)^2 / vx_dm) / 2,    -inf for w_m <= 0
    p_tm = exp(l_tm - u_t) / sum_k exp(l_tk - u_t),  u_t = max_m l_tm
    y_dt = sum_m p_tm (muy_dm + a_dm (x_dt - mux_dm)),  a_dm = c_dm / vx_dm

Bounds (eps = 2^-53, the unit roundoff of float64; starred quantities exact):

 * log-density, the issue's: B_tm = (D + 16) eps (1/2 sum_d dx^2 / vx + |log w_m| + 1/2 sum_d |log vx_dm|).  The centred sum
   q = sum_d fl(dx^2) fl(1 / vx) has D terms of relative error <= 4 eps (dx, its square, the reciprocal, the product inside the
   fma) accumulated with <= D roundings: (D + 4) eps q; the constant is a sum of D + 2 terms: (D + 4) eps of their absolute
   sum; the final subtraction one more.  (D + 16) covers all of it with room for the library's log.
 * posterior, the issue's: max_m |dP_tm| <= 2 max_m B_tm + (M + 16) eps -- l_m - u carries B_m + B_u, exp turns an absolute
   error into a relative one, p <= 1; the sum of M terms, the quotient and exp's own error are the (M + 16) eps.
 * y, for the form the kernel evaluates -- per mixture e_dm = fma(a_dm, fl(x_d - mux_dm), muy_dm), then M chained
   y <- fma(p_m, e_dm, y):
       |d e_dm|  <= 3 eps (|muy_dm| + |a_dm dx_dm|)        (the difference, the quotient a = fl(c / vx), the fma)
       |d y_dt|  <= sum_m |dP_tm| |e_dm|  +  sum_m p_tm |d e_dm|  +  (M + 1) eps sum_m p_tm |e_dm|
                 <= PB_t sum_m |e_dm|  +  (M + 4) eps sum_m p_tm (|muy_dm| + |a_dm dx_dm|)
   with PB_t the posterior bound above.  The first term is the loose one (an absolute bound of dP against every |e_dm|)."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53

# (D, M, T) of the parity test: the smallest; odd D, a tile and a frame; neither fills anything; odd D past 40, a prime M, T past
# four tiles; the headline shape, T past 64 tiles and off the tile; delta features; the largest D; the largest M ...
PARITY_SHAPES = [(1, 1, 5), (3, 2, 65), (25, 5, 130), (41, 17, 257), (40, 64, 4099), (80, 32, 200), (128, 3, 70), (8, 256, 64)]
# ... and the shapes at which the kernel runs its 32-frame tiles (D and M both large), up to the limits
SMALL_TILE_SHAPES = [(101, 129, 70), (128, 256, 33)]


def split(w, mu, covars, swap=False, dtype=np.float64):
    """-> w (M,), mux, muy, vx, a (D,M) in dtype"""
    w, mu, cov = (np.asarray(a, dtype=dtype) for a in (w, mu, covars))
    D = mu.shape[0] // 2
    mux, muy, vx, vy, c = mu[:D], mu[D:], cov[:D], cov[D:2 * D], cov[2 * D:]
    if swap:
        mux, muy, vx = muy, mux, vy
    return w, mux, muy, vx, c / vx


def logdens(X, w, mu, covars, swap=False, dtype=np.float64):
    """(T,M) log w_m + log N(x_t; mux_m, diag vx_m), centred; -inf where w_m <= 0"""
    w, mux, muy, vx, a = split(w, mu, covars, swap, dtype)
    X = np.asarray(X, dtype=dtype)
    D, M = mux.shape
    log2pi = np.log(2 * np.arccos(dtype(-1)))
    L = np.full((X.shape[0], M), -np.inf, dtype=dtype)
    for m in range(M):
        if not w[m] > 0:
            continue
        dx = X - mux[:, m]
        L[:, m] = np.log(w[m]) - (D * log2pi + np.log(vx[:, m]).sum() + (dx * dx / vx[:, m]).sum(axis=1)) / 2
    return L


def posterior(L):
    u = L.max(axis=1, keepdims=True)
    E = np.exp(L - u)
    return E / E.sum(axis=1, keepdims=True)


def convert(X, w, mu, covars, swap=False, dtype=np.float64):
    """-> Y (T,D), P (T,M), L (T,M) in dtype"""
    wv, mux, muy, vx, a = split(w, mu, covars, swap, dtype)
    X = np.asarray(X, dtype=dtype)
    L = logdens(X, w, mu, covars, swap, dtype)
    P = posterior(L)
    Y = np.zeros_like(X)
    for m in range(mux.shape[1]):
        Y += P[:, m:m + 1] * (muy[:, m] + a[:, m] * (X - mux[:, m]))
    return Y, P, L


def predict(L):
    """1-based first maximum"""
    return np.argmax(np.asarray(L, dtype=np.float64), axis=1).astype(np.int64) + 1


def logdens_bound(X, w, mu, covars, swap=False):
    """B (T,M), float64; +inf where w_m <= 0 (no statement: both sides are -inf there)"""
    w, mux, muy, vx, a = split(w, mu, covars, swap, LD)
    X = np.asarray(X, dtype=LD)
    D, M = mux.shape
    B = np.full((X.shape[0], M), np.inf)
    for m in range(M):
        if not w[m] > 0:
            continue
        dx = X - mux[:, m]
        B[:, m] = (D + 16) * EPS * ((dx * dx / vx[:, m]).sum(axis=1) / 2 + abs(np.log(w[m])) + np.abs(np.log(vx[:, m])).sum() / 2)
    return B


def posterior_bound(X, w, mu, covars, swap=False):
    """PB (T,): max_m |P_tm - P*_tm| <= 2 max_m B_tm + (M + 16) eps, the maximum over the mixtures with w_m > 0"""
    B = logdens_bound(X, w, mu, covars, swap)
    M = B.shape[1]
    return 2 * np.where(np.isfinite(B), B, 0.0).max(axis=1) + (M + 16) * EPS


def convert_bound(X, w, mu, covars, swap=False):
    """YB (T,D) for the kernel's form (module docstring), from the longdouble model"""
    wv, mux, muy, vx, a = split(w, mu, covars, swap, LD)
    X = np.asarray(X, dtype=LD)
    _, P, _ = convert(X, w, mu, covars, swap, LD)
    PB = posterior_bound(X, w, mu, covars, swap)[:, None]
    M = mux.shape[1]
    sum_e, sum_pe = np.zeros_like(X), np.zeros_like(X)
    for m in range(M):
        adx = a[:, m] * (X - mux[:, m])
        sum_e += np.abs(muy[:, m] + adx)
        sum_pe += P[:, m:m + 1] * (np.abs(muy[:, m]) + np.abs(adx))
    return np.asarray(PB * sum_e + (M + 4) * EPS * sum_pe, dtype=np.float64)


def cancellation_case(T=2000, D=8):
    """Where an expanded log-density cancels: four mixtures whose source means differ by 0.5e-3 at |mean| ~ 10 and variances
    ~1e-6 (x^2 / v ~ 1e8 against differences of order 1), target side mu_y = -mu_x with variances of the same size and pair
    correlations alternating +-0.9; frames drawn from the model.  -> w, mu (2D,M), covars (3D,M), X (T,2D) joint frames"""
    from em_bdiag_restatement import draw
    rng = np.random.default_rng(77)
    M = 4
    w = np.array([0.1, 0.2, 0.3, 0.4])
    m1 = 10.0 * np.where(rng.random(D) < 0.5, -1.0, 1.0) + 0.1 * rng.standard_normal(D)
    mux = m1[:, None] + 0.5e-3 * rng.standard_normal((D, M))
    vx = 1e-6 * np.exp(0.1 * rng.standard_normal((D, M)))
    vy = 1e-6 * np.exp(0.1 * rng.standard_normal((D, M)))
    rho = 0.9 * np.where(np.arange(D) % 2 == 0, 1.0, -1.0)[:, None]
    mu = np.asfortranarray(np.vstack([mux, -mux]))
    cov = np.asfortranarray(np.vstack([vx, vy, rho * np.sqrt(vx * vy)]))
    return w, mu, cov, draw(78, w, mu, cov, T)


def expanded_posterior(X, w, mu, covars):
    """the UNCORRECTED expanded form x^2 (1/v) - 2 x (mu/v) + mu^2/v as products in float64: what the device must not compute
    (the host test shows that it misses the posterior bound on cancellation_case)"""
    wv, mux, muy, vx, a = split(w, mu, covars, False, np.float64)
    X = np.asarray(X, dtype=np.float64)
    D = mux.shape[0]
    q = (X * X) @ (1 / vx) - 2 * X @ (mux / vx) + (mux * mux / vx).sum(axis=0)
    return posterior(np.log(wv) - (D * np.log(2 * np.pi) + np.log(vx).sum(axis=0) + q) / 2)
