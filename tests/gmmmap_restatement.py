"""Restatement of frame-by-frame conversion with a full-covariance joint GMM (test helper, not a test module): GMMMap
fvconvert / predict_proba / predict (csrc/gmmmap.hip, csrc/gmmmap_fallback.hip, csrc/gmmmap_screen.hpp) in numpy longdouble,
straight from (w, mu, Sigma), independent of the library and of the oracles; the error bounds
tests/test_gpu_gmmmap_shared.py holds the device to; and two model generators whose frames SHARE their posterior among the
mixtures.  tests/test_gmmmap_restatement_host.py checks this file against oracle/np_oracle.GMMMap and oracle/c_oracle.GMMMap
and asserts the generators' properties before the device is judged by it.

Arrays follow the oracles: w (M,); mu (M,Dj); sigma (M,Dj,Dj) indexed [m][col][row] (the Julia memory image), D = Dj / 2.
Frames X (T,D), results Y (T,D), P (T,M), L (T,M).

The model, source side x and target side y (swap exchanges the halves), L_m the lower Cholesky factor of Hermitian(Sxx_m):
    l_tm = log w_m - (D log 2 pi + log det Sxx_m + |inv(L_m) (x_t - mux_m)|^2) / 2,          -inf for w_m <= 0
    p_tm = exp(l_tm - u_t) / sum_k exp(l_tk - u_t),  u_t = max_m l_tm;   predict = the first maximum, 1-based
    y_t  = sum_m p_tm e_tm,   e_tm = muy_m + Syx_m inv(Sxx_m) (x_t - mux_m)

Bounds (eps = 2^-53, the unit roundoff of float64; starred quantities exact; first order in eps; absolute values and
inequalities of vectors and matrices are meant element by element).  The device evaluates, from quantities the host
prepares once in float64 (csrc/gmmmap_prepare.cpp),
    l = lc - |U x - cz|^2 / 2,   U = inv(L), cz = U mux, lc = log w - (D log 2 pi + 2 sum_i log L_ii) / 2
    y = sum_m p_m (A_m x + b_m),  A = Syx inv(Sxx) (Gauss-Jordan on the raw block), b = muy - A mux
With z = U (x - mux), s = |U| (|x| + |mux|), K = |U| |L|:

 * log-density, every term with its own count of roundings:
       B_tm = eps ((2 D + 2) |z|.s + D |z|.(K s) + (D + 1) |K'|z||^2 / 2 + (D + 4) |z|^2 / 2 + (D + 1) |K|_F^2 / 2
                   + 2 |log w| + (D + 2) sum_i |log L_ii| + 2 D log(2 pi) / 2 + 3 (|log w| + D log(2 pi) / 2 + sum_i |log L_ii| + |z|^2 / 2))
     - the whitening on the device: z_i starts from -cz_i and takes up to D fused multiply-adds in whatever order the matrix
       pipe sums them, plus the addition of two accumulator chains: |dz_i| <= (D + 2) eps (|U| |x| + |cz|)_i <= (D + 2) eps s_i;
       cz = fl(U mux) on the host, D products and D additions: |d cz_i| <= D eps (|U| |mux|)_i <= D eps s_i.  dl = z.dz:
       (2 D + 2) eps |z|.s, the first term;
     - the triangular inverse (column by column substitution): |fl(U) L - I| <= D eps |U| |L|, so |dU| <= D eps |U| |L| |U| and,
       applied to x and to mux separately, |dz| <= D eps K s: the second term;
     - the Cholesky factorisation: fl(L) fl(L)' = Sxx + dS with |dS| <= (D + 1) eps |L| |L'| (Higham, Accuracy and Stability,
       theorem 10.3).  d|z|^2 = (U'z)' dS (U'z), at most (D + 1) eps |K'|z||^2: the third term after the factor 1/2; and
       d log det = tr(inv(Sxx) dS) = tr(U dS U') <= (D + 1) eps |K|_F^2: the fifth.  This is where the conditioning of L_m
       enters: K is the identity for a diagonal L and grows with cond(L);
     - |z|^2 summed by D fused multiply-adds and the exchange among four lanes: (D + 4) eps |z|^2, halved: the fourth;
     - lc: log w with a relative error of 2 eps; D logarithms of 2 eps each summed by D additions: (D + 2) eps sum |log L_ii|;
       the constant log 2 pi and its product with D: 2 eps D log(2 pi) / 2;
     - the two additions that assemble lc and the final l = lc - q / 2: three roundings of at most
       eps (|log w| + D log(2 pi) / 2 + sum |log L_ii| + |z|^2 / 2) each.
   The second-order terms are below D eps cond(L)^2 < 1e-9 of B at the conditionings used here: B is multiplied by 1 + 2^-20.
 * posterior, relative: log p_m = l_m - lse, lse = log sum_k exp l_k, d lse = sum_k p_k dl_k <= max_k B_k.  The softmax itself,
   as posterior_finish_kernel evaluates it, p_m = exp(l_m - u) (1 / s), u = max_k l_k, s = sum_k exp(l_k - u): the difference
   l_m - u rounds with eps |l_m - u| <= eps (|log P*_m| + log M), and exp turns that into a relative error; the sum of M terms
   in any order, two exponentials (argument reduction exact for |n| < 2^11, polynomial good to 2 eps), the reciprocal and the
   product are (M + 16) eps.  (The form exp(l_m - (u + log s)) of src/gmm.jl:28-29, which the oracles keep, rounds lse as
   well: eps |lse|, which the three final roundings counted in max_k B_k cover.)  So
       |log P_tm - log P*_tm| <= B_tm + max_k B_tk + (M + 16) eps + eps (|log P*_tm| + log M) =: Q_tm + max_k B_tk.
   posterior_bound returns R (T,M): that where P* <= 1e-3 and with B_tm replaced by max_k B_tk elsewhere, as a bound on
   |P / P* - 1|, stated for P* >= 1e-300 (the maximum runs over the mixtures with w_m > 0); and
   PB (T,) = 2 max_k B_tk + (M + 16 + log M) eps, which bounds |P - P*| absolutely since P |log P| <= 1.
 * y, with h_dm = (|A_m| (|x| + |mux_m|))_d + |muy_dm| (it bounds |A x| + |b| and |e_dm|) and
   g_dm = (G_m (|x| + |mux_m|))_d, G = |Syx| |inv Sxx| (I + |Sxx| |inv Sxx|):
     |dy_d| <= sum_m p_m R_tm |e_dm|                           (the relative error of every posterior; the form
                                                                PB_t sum_m |e_dm| of tests/gmmmap_bdiag_restatement.py is
                                                                this one with p_m <= 1 and R_tm <= PB_t: M times looser)
             + (2 M + 2 D + 32) eps sum_m p_m h_dm             (M fused multiply-adds y <- fma(w_m, e_m, y sc), as many
                                                                rescalings and the final quotient: 2 M + 2; e = b + A x by D
                                                                fused multiply-adds: D + 1; b = muy - fl(A mux): D + 1)
             + (2 D + 16) eps sum_m p_m g_dm                   (A: an element of the Gauss-Jordan inverse takes D updates of
                                                                two roundings and a division, amplified by |inv S| |S|:
                                                                |d inv S| <= (2 D + 1) eps |inv S| |S| |inv S|, no pivot
                                                                growth for a positive definite block; the product
                                                                Syx inv S: D eps |Syx| |inv S|)
             + e^-prune (sum_m |e_dm| + M sum_m p_m |e_dm|)    (a mixture whose posterior is below e^-prune of the running
                                                                maximum may be left out of y, and of the denominator:
                                                                y' - y = sum_S p_m (y - e_m) / (1 - p_S))
   The first term is the largest: R carries the conditioning of L_m.

The bounds are computed in float64 from the longdouble model; their own rounding is a relative 1e-14 of themselves.

Generators (their properties are asserted by tests/test_gmmmap_restatement_host.py):
 * tied_model: every mixture shares one orthogonal Q and one spectrum up to a jitter, and the means lie within the spread of
   the covariances: the posterior of a frame drawn from the model is shared among several mixtures.
 * source_tied_ladder: the mixtures have a bit-identical source side, so the posterior of EVERY frame is the normalised
   weight vector itself -- known without any reference arithmetic, down to 7e-305 -- and y = sum_m w_m e_m needs no
   exponential."""
import numpy as np
import scipy.linalg as sla

from em_restatement import LD, LOG2PI, chol

EPS = 2.0 ** -53
PRUNE = 46.0                                   # the library's default threshold, nats

# (D, M, T) per kernel path of tests/test_gpu_gmmmap_shared.py; every T is off the 16-, 64- and 128-frame tiles
GENERIC_SHAPES = [(7, 3, 131)]                                                        # + (40, 9) through set_kernel(1)
TILE_SHAPES = [(D, M, 131) for D in (13, 16, 25, 40, 48) for M in (3, 9, 64)]         # one wave per tile, DP <= 48
WIDE_TILE_DIMS = (16, 40, 48)                                                         # two tiles per wave on top
EIGHT_WAVE_SHAPES = [(D, M, 197) for D in (50, 56, 57, 64, 72, 75, 80) for M in (4, 6)]
FALLBACK_SHAPES = [(82, 5, 150), (100, 5, 150), (160, 5, 150), (130, 70, 133)]
GROUPED_SHAPES = [(24, 9, 8192 + 7), (48, 9, 8192 + 7)]
SETTINGS = {"default": dict(jitter=0.05, spread=1.0), "hard": dict(jitter=0.1, spread=2.0)}
POSTERIOR_DIMS = (7, 40, 56, 80, 100, 160)
POSTERIOR_MS = (8, 9, 16, 17, 32, 33, 64, 65, 130)
POSTERIOR_TIED_SHAPES = [(D, M) for D in POSTERIOR_DIMS for M in POSTERIOR_MS]


def posterior_checked_frames(D, M, T=131):
    """The frames of a tied-model posterior case that are compared with the longdouble reference: all T where the reference
    takes a second or two, else the first 13 (the short call) and every fourth of the rest.  The device computes all T."""
    if M * D * D <= 65 * 100 * 100:
        return np.arange(T)
    return np.unique(np.concatenate([np.arange(13), np.arange(13, T, 4)]))
LADDER_GAPS = (47.0, 0.0, 1.0, 20.0, 45.0, 300.0, 700.0)
LADDER_ORDERS = {"first": (0.0, 1.0, 20.0, 45.0, 47.0, 300.0, 700.0), "middle": (47.0, 20.0, 1.0, 0.0, 45.0, 300.0, 700.0),
                 "last": (700.0, 300.0, 47.0, 45.0, 20.0, 1.0, 0.0)}
LADDER_TIED = (47.0, 0.0, 1.0, 0.0, 20.0, 45.0, 300.0, 700.0)      # mixtures 2 and 4 (1-based) tie bit for bit: predict = 2


# ------------------------------------------------------------------------------------------------------------ generators
def tied_model(seed, Dj, M, lam_lo=1e-3, jitter=0.05, spread=1.0):
    """One orthogonal Q and one spectrum lam (log-uniform in [lam_lo, 1]) for all mixtures:
    Sigma_m = Q diag(lam exp(jitter n_m)) Q', symmetrised; mu_m = mu_0 + spread / sqrt(Dj / 2) Q diag(sqrt lam) n'_m;
    Dirichlet(2) weights.  -> w (M,), mu (M,Dj), sigma (M,Dj,Dj)"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((Dj, Dj)))
    lam = np.exp(rng.uniform(np.log(lam_lo), 0.0, Dj))
    mu0 = rng.standard_normal(Dj)
    w = rng.dirichlet(2.0 * np.ones(M))
    mu = np.empty((M, Dj))
    sig = np.empty((M, Dj, Dj))
    for m in range(M):
        S = (Q * (lam * np.exp(jitter * rng.standard_normal(Dj)))) @ Q.T
        sig[m] = (S + S.T) / 2.0
        mu[m] = mu0 + spread / np.sqrt(Dj / 2.0) * (Q @ (np.sqrt(lam) * rng.standard_normal(Dj)))
    return w, mu, sig


def source_tied_ladder(seed, D, gaps, lam_lo=1e-2):
    """len(gaps) mixtures with the source side (mux, Sxx) of ONE synth_model(seed, 2 D, 1, lam_lo), bit for bit; target
    means shifted by N(0,1); Sigma_m = diag(I, s_m I) Sigma diag(I, s_m I) with s_m uniform in [1, 1.3] (positive definite
    with Sigma); weights proportional to exp(-gaps).  -> w (M,), mu (M,2D), sigma (M,2D,2D)"""
    from synthdata import synth_model
    w1, mu1, sig1 = synth_model(seed, 2 * D, 1, lam_lo=lam_lo)
    rng = np.random.default_rng(seed + 1)
    gaps = np.asarray(gaps, dtype=np.float64)
    M = len(gaps)
    w = np.exp(-gaps)
    w = w / w.sum()
    mu = np.repeat(mu1, M, axis=0)
    sig = np.repeat(sig1, M, axis=0)
    for m in range(M):
        s = rng.uniform(1.0, 1.3)
        mu[m, D:] += rng.standard_normal(D)
        sig[m, D:, :D] *= s
        sig[m, :D, D:] *= s
        sig[m, D:, D:] *= s * s
    return w, mu, sig


def ladder_gaps(M, gaps=LADDER_GAPS):
    """the ladder repeated up to M mixtures"""
    return tuple((gaps * (-(-M // len(gaps))))[:M])


def frames(seed, w, mu, sig, T, swap=False):
    """T frames drawn from the model's own p(x)"""
    from synthdata import sample_frames
    D = mu.shape[1] // 2
    return sample_frames(seed, w, mu, sig, T, D if swap else 0, 2 * D if swap else D)


# ------------------------------------------------------------------------------------------------------- the restatement
def _inverse(S):
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


def _forward(L, B):
    """inv(L) B by forward substitution in longdouble; B (D,T)"""
    Z = np.empty_like(B)
    for i in range(L.shape[0]):
        Z[i] = (B[i] - L[i, :i] @ Z[:i]) / L[i, i]
    return Z


class Model:
    """The longdouble pieces of a model, per mixture: mux, muy (D,), L, A = Syx inv(Sxx), and what the bounds need.
    Mixtures with bit-identical source (and cross) blocks share their factorisations."""

    def __init__(self, w, mu, sigma, swap=False):
        self.w = np.asarray(w, dtype=np.float64)
        mu = np.asarray(mu, dtype=np.float64)
        S = np.transpose(np.asarray(sigma, dtype=np.float64), (0, 2, 1))          # [m][row][col]
        self.M, Dj = mu.shape
        self.D = D = Dj // 2
        xs, ys = (slice(D, 2 * D), slice(0, D)) if swap else (slice(0, D), slice(D, 2 * D))
        self.mux, self.muy = mu[:, xs].astype(LD), mu[:, ys].astype(LD)
        self.Sxx, self.Syx = S[:, xs, xs], S[:, ys, xs]
        self._fact, self._inv, self._A = {}, {}, {}

    def fact(self, m):
        """-> L (longdouble); |U|, U = inv(L), and K = |U| |L| in float64 (they enter the bounds only)"""
        key = self.Sxx[m].tobytes()
        if key not in self._fact:
            L = chol(self.Sxx[m])
            L64 = L.astype(np.float64)
            Ua = np.abs(sla.solve_triangular(L64, np.eye(self.D), lower=True))
            self._fact[key] = (L, Ua, Ua @ np.abs(L64))
        return self._fact[key]

    def slope(self, m):
        """-> A = Syx inv(Sxx) (longdouble), G = |Syx| |inv Sxx| (I + |Sxx| |inv Sxx|) (float64)"""
        key = self.Sxx[m].tobytes() + self.Syx[m].tobytes()
        if key not in self._A:
            if key[:self.Sxx[m].nbytes] not in self._inv:
                self._inv[key[:self.Sxx[m].nbytes]] = _inverse(self.Sxx[m])
            Sinv = self._inv[key[:self.Sxx[m].nbytes]]
            a = np.abs(Sinv).astype(np.float64)
            G = np.abs(self.Syx[m]) @ a @ (np.eye(self.D) + np.abs(self.Sxx[m]) @ a)
            self._A[key] = (self.Syx[m].astype(LD) @ Sinv, G)
        return self._A[key]

    def lc_parts(self, m):
        """|log w|, D log(2 pi) / 2, sum |log L_ii|"""
        L = self.fact(m)[0]
        return float(abs(np.log(LD(self.w[m])))), float(self.D * LOG2PI / 2), float(np.abs(np.log(np.diag(L))).sum())

    # -------------------------------------------------------------------------------------------------------- values
    def whiten(self, X, m):
        """z (T,D) = inv(L_m) (x - mux_m) by forward substitution in longdouble"""
        return _forward(self.fact(m)[0], (np.asarray(X, dtype=LD) - self.mux[m]).T).T

    def logdens(self, X):
        """L (T,M) longdouble; -inf where w_m <= 0"""
        out = np.full((len(X), self.M), -np.inf, dtype=LD)
        zcache = {}
        for m in range(self.M):
            if not self.w[m] > 0:
                continue
            key = self.Sxx[m].tobytes() + self.mux[m].tobytes()
            if key not in zcache:
                Z = self.whiten(X, m)
                zcache[key] = (Z * Z).sum(axis=1)
            Lm = self.fact(m)[0]
            out[:, m] = np.log(LD(self.w[m])) - (self.D * LOG2PI + 2 * np.log(np.diag(Lm)).sum() + zcache[key]) / 2
        return out

    def regress(self, X, m):
        """e_m (T,D) = muy_m + (x - mux_m) A_m'"""
        return self.muy[m] + (np.asarray(X, dtype=LD) - self.mux[m]) @ self.slope(m)[0].T

    def convert(self, X):
        """-> Y (T,D), P (T,M), L (T,M) in longdouble"""
        L = self.logdens(X)
        P = posterior(L)
        Y = np.zeros((len(X), self.D), dtype=LD)
        for m in range(self.M):
            if self.w[m] > 0:
                Y += P[:, m:m + 1] * self.regress(X, m)
        return Y, P, L

    # -------------------------------------------------------------------------------------------------------- bounds
    def logdens_bound(self, X):
        """B (T,M), float64; +inf where w_m <= 0 (no statement: both sides are -inf there)"""
        X64 = np.asarray(X, dtype=np.float64)
        D = self.D
        B = np.full((len(X), self.M), np.inf)
        cache = {}
        for m in range(self.M):
            if not self.w[m] > 0:
                continue
            key = self.Sxx[m].tobytes() + self.mux[m].tobytes()
            if key not in cache:
                L, Ua, K = self.fact(m)
                z = np.abs(self.whiten(X, m)).astype(np.float64)
                s = (np.abs(X64) + np.abs(self.mux[m]).astype(np.float64)) @ Ua.T
                kz = z @ K                                                 # (K'|z|)' per frame
                q2 = (z * z).sum(axis=1) / 2
                cache[key] = ((2 * D + 2) * (z * s).sum(axis=1) + D * (z * (s @ K.T)).sum(axis=1) + (D + 1) * (kz * kz).sum(axis=1) / 2
                              + (D + 4) * q2 + (D + 1) * (K * K).sum() / 2, q2)
            lw, l2pi, ld = self.lc_parts(m)
            B[:, m] = (1 + 2.0 ** -20) * EPS * (cache[key][0] + 2 * lw + (D + 2) * ld + 2 * l2pi + 3 * (lw + l2pi + ld + cache[key][1]))
        return B

    def posterior_bound(self, X, P=None):
        """-> R (T,M) on |P / P* - 1| (where P* >= 1e-300), PB (T,) on |P - P*|; see the module docstring"""
        B = self.logdens_bound(X)
        if P is None:
            P = posterior(self.logdens(X))
        Bf = np.where(np.isfinite(B), B, 0.0)
        bmax = Bf.max(axis=1, keepdims=True)
        P64 = np.asarray(P, dtype=np.float64)
        logp = np.abs(np.log(np.maximum(P64, 1e-300)))
        R = np.where(P64 <= 1e-3, Bf + bmax, 2 * bmax) + (self.M + 16 + np.log(self.M) + logp) * EPS
        return R, 2 * bmax[:, 0] + (self.M + 16 + np.log(self.M)) * EPS

    def convert_bound(self, X, prune=PRUNE):
        """YB (T,D), float64, for y = sum p (A x + b) with mixtures below e^-prune left out (prune = inf: none)"""
        X64 = np.asarray(X, dtype=np.float64)
        P = np.asarray(posterior(self.logdens(X)), dtype=np.float64)
        R, _ = self.posterior_bound(X, P)
        D, M = self.D, self.M
        sum_e, sum_pe, sum_pre, sum_ph, sum_pg = (np.zeros((len(X), D)) for _ in range(5))
        for m in range(M):
            if not self.w[m] > 0:
                continue
            A, G = self.slope(m)
            e = np.abs(self.regress(X, m)).astype(np.float64)
            ax = np.abs(X64) + np.abs(self.mux[m]).astype(np.float64)
            sum_e += e
            sum_pe += P[:, m:m + 1] * e
            sum_pre += (P[:, m:m + 1] * R[:, m:m + 1]) * e
            sum_ph += P[:, m:m + 1] * (ax @ np.abs(A).astype(np.float64).T + np.abs(self.muy[m]).astype(np.float64))
            sum_pg += P[:, m:m + 1] * (ax @ G.T)
        return (sum_pre + (2 * M + 2 * D + 32) * EPS * sum_ph + (2 * D + 16) * EPS * sum_pg
                + np.exp(-prune) * (sum_e + M * sum_pe))


def posterior(L):
    """max-shifted softmax along the mixtures"""
    u = L.max(axis=1, keepdims=True)
    E = np.exp(L - u)
    return E / E.sum(axis=1, keepdims=True)


def predict(L):
    """1-based first maximum (decided in the precision L comes in)"""
    return np.argmax(L, axis=1).astype(np.int64) + 1


def convert(X, w, mu, sigma, swap=False):
    """-> Y (T,D), P (T,M), L (T,M) in longdouble"""
    return Model(w, mu, sigma, swap).convert(X)


def logdens_bound(X, w, mu, sigma, swap=False):
    return Model(w, mu, sigma, swap).logdens_bound(X)


def posterior_bound(X, w, mu, sigma, swap=False):
    return Model(w, mu, sigma, swap).posterior_bound(X)


def convert_bound(X, w, mu, sigma, swap=False, prune=PRUNE):
    return Model(w, mu, sigma, swap).convert_bound(X, prune)


def ladder_posterior(w):
    """the posterior of every frame of a source-tied ladder: w / sum(w) in longdouble"""
    wl = np.asarray(w, dtype=LD)
    return wl / wl.sum()


def ladder_convert(X, w, mu, sigma, swap=False):
    """y = sum_m w_m e_m(x) in longdouble -- no exponential, no logarithm"""
    mdl = Model(w, mu, sigma, swap)
    p = ladder_posterior(w)
    Y = np.zeros((len(X), mdl.D), dtype=LD)
    for m in range(mdl.M):
        Y += p[m] * mdl.regress(X, m)
    return Y


def shared_frames(P, level=1e-3):
    """-> the share of frames whose second largest posterior is >= level, and of those whose third is (nan for M < 3)"""
    Ps = np.sort(np.asarray(P, dtype=np.float64), axis=1)
    return float(np.mean(Ps[:, -2] >= level)), float(np.mean(Ps[:, -3] >= level)) if Ps.shape[1] >= 3 else float("nan")
