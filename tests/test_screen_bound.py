"""CPU: the two inequalities the screen of fvconvert's shape 3 rests on (csrc/gmmmap_screen.hpp), checked numerically with
numpy emulations -- no GPU, no library call:
  (1) a partial sum of the eigen-expansion of (x - mu)' inv(S) (x - mu) over the largest eigenpairs of inv(S) is a lower
      bound of it (so lc - bound / 2 is an upper bound of the mixture's log-density);
  (2) the bf16-split evaluation  a^ = Ph xh + Ph xl + Pl xh - c  with FP32 accumulation differs from a = P x - c by at most
      eps = 2^-12 (|P| |x| + |c|) -- the margin the kernel subtracts from |a^| before squaring -- also under heavy
      cancellation (c thousands of times a) and for any summation order."""
import numpy as np
import pytest


def bf16_round(x32):
    """float32 -> nearest bf16 (ties to even), returned as float32 (the kernel's split_bf16)."""
    u = np.asarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return r.astype(np.uint32).view(np.float32)


def split(x64):
    xf = np.asarray(x64, dtype=np.float64).astype(np.float32)
    hi = bf16_round(xf)
    lo = bf16_round((xf - hi).astype(np.float32))        # xf - hi is exact in float32
    return hi, lo


def test_partial_eigen_sum_is_a_lower_bound():
    rng = np.random.default_rng(0)
    for D in (16, 24, 40):
        for _ in range(20):
            Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
            lam = np.exp(rng.uniform(np.log(1e-5), 0.0, D))
            S = (Q * lam) @ Q.T
            S = 0.5 * (S + S.T)
            Sinv = np.linalg.inv(S)
            kap, V = np.linalg.eigh(Sinv)
            order = np.argsort(kap)[::-1]
            P = (np.sqrt(kap[order[:4]])[:, None] * V[:, order[:4]].T)          # rows sqrt(kappa_i) v_i'
            mu = rng.standard_normal(D)
            X = mu + rng.standard_normal((200, D)) * rng.uniform(0.01, 3.0, (200, 1))
            full = np.einsum("td,de,te->t", X - mu, Sinv, X - mu)
            for rows in (1, 2, 4):
                part = (((X - mu) @ P[:rows].T) ** 2).sum(1)
                assert np.all(part <= full * (1 + 1e-9) + 1e-9)


def test_bf16_split_error_margin_holds():
    rng = np.random.default_rng(1)
    worst = 0.0
    for D in (16, 28, 40):
        for scale_p, shift in ((1.0, 0.0), (300.0, 0.0), (300.0, 500.0), (3.0, -2000.0), (1e3, 50.0)):
            P = rng.standard_normal((64, D)) * scale_p * np.exp(rng.uniform(-3, 0, (64, 1)))
            mu = rng.standard_normal(D) + shift
            X = mu + rng.standard_normal((256, D)) * rng.uniform(1e-3, 2.0, (256, 1))
            c = P @ mu
            a = X @ P.T - c                                                       # (T, rows), float64: the quantity bounded
            ph, pl = split(P)
            xh, xl = split(X)
            # the products of two bf16 numbers are exact in float32; accumulate the 3 D terms in float32, in two different orders
            terms = np.concatenate([xh[:, None, :] * ph[None], xl[:, None, :] * ph[None], xh[:, None, :] * pl[None]], axis=2).astype(np.float32)
            for order in (slice(None), slice(None, None, -1)):
                acc = (-c).astype(np.float32)[None, :] * np.ones((X.shape[0], 1), np.float32)
                for k in range(terms.shape[2])[order]:
                    acc = (acc + terms[:, :, k]).astype(np.float32)
                eps = 2.0 ** -12 * (np.linalg.norm(P, axis=1)[None, :] * np.linalg.norm(X, axis=1)[:, None] + np.abs(c)[None, :])
                err = np.abs(acc.astype(np.float64) - a)
                assert np.all(err <= eps), float((err / eps).max())
                worst = max(worst, float((err / eps).max()))
                # ... hence the certified lower bound of a^2 never exceeds a^2
                lb = np.maximum(np.abs(acc.astype(np.float64)) - eps, 0.0) ** 2
                assert np.all(lb <= a * a * (1 + 1e-12) + 1e-300)
    assert worst < 0.6          # the margin is about twice what the arithmetic needs (sequential FP32 accumulation, the worst order)


# ---- the E-step's hard-assignment key (csrc/estep_hard.hpp): estep_hard_prep_kernel + the rule of estep_hard_key_kernel ----
#
# A frame is HARD (one responsibility exactly 1, every other exactly 0) when  second + E < (best - E) - 746  for the two largest
# bf16-split log-densities l^ of the frame, E = NWmax |[x^2 ; x]| + NCmax, and every operand stays inside the kernel's finite
# range (kHardFinite).  The emulation reproduces the kernel's arithmetic -- the splits, c and the margins in float with up() and
# the (1 + 2^-20) / 1.000001 factors, FP32 accumulation of the exact bf16 products in three orders -- and every frame it
# declares hard is checked against an extended-precision evaluation: the true gap exceeds 745.2 nats (exp of anything below
# -745.14 is exactly 0 in FP64) and the owner is the true arg-max.

F32 = np.float32
HARD_FINITE = F32(2.0 ** 114)
LOG2PI = np.log(2.0 * np.pi)


def _split_nonfinite(x64):
    """split() for values that may leave the float32 range (-inf hi, NaN lo), as split_bf16 / v_cvt_pk_bf16_f32 give them"""
    with np.errstate(over="ignore", invalid="ignore"):
        xf = np.asarray(x64, dtype=np.float64).astype(np.float32)
        u = xf.view(np.uint32).astype(np.uint64)
        hi = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
        r = (xf - hi).astype(np.float32)
        v = r.view(np.uint32).astype(np.uint64)
        lo = (((v + 0x7FFF + ((v >> 16) & 1)) >> 16 << 16) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    return hi, lo


def _up(v, finite_range=True):
    """the prep kernel's up(): the next float above v (1 + 2^-20), infinite for NaN and from kHardFinite on"""
    if finite_range and not v < float(HARD_FINITE):
        return F32(np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.array(np.float64(v) * (1.0 + 2.0 ** -20), dtype=np.float32)
    return (f.view(np.uint32) + np.uint32(1)).view(np.float32)[()]


def hard_prep(w, mu, var, finite_range=True):
    """(Wh, Wl (Mp, 2 dj) float32, c (Mp,) float32, NW, NC (Mp,)): the mixture tiles of estep_hard_prep_kernel, padded to 16"""
    M, dj = mu.shape
    Mp = 16 * ((M + 15) // 16)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        ivv = 1.0 / var
        Wd = np.concatenate([-0.5 * ivv, mu * ivv], axis=1)
        logw = np.where(w > 0, np.log(np.where(w > 0, w, 1.0)), -np.inf)
        c = logw - 0.5 * (dj * LOG2PI + np.log(var).sum(1)) - 0.5 * (mu * mu * ivv).sum(1)
        q = ((0.5 * ivv) ** 2 + (mu * ivv) ** 2).sum(1)
    Wh, Wl = np.zeros((Mp, 2 * dj), F32), np.zeros((Mp, 2 * dj), F32)
    Wh[:M], Wl[:M] = _split_nonfinite(Wd)
    cf, nw, nc = np.full(Mp, -1e30, F32), np.zeros(Mp, F32), np.zeros(Mp, F32)
    for m in range(M):
        if c[m] != -np.inf:                        # weight 0: dead (c = -1e30, margins 0)
            with np.errstate(over="ignore", invalid="ignore"):
                cf[m] = F32(c[m])
            nw[m] = _up(np.sqrt(q[m]) * 2.0 ** -12, finite_range)
            nc[m] = _up(abs(c[m]) * 2.0 ** -12, finite_range)
    return Wh, Wl, cf, nw, nc


def hard_keys(w, mu, var, X, order, line=746.0, three_terms=True, finite_range=True):
    """estep_hard_key_kernel's key of every frame (M = soft).  order: 'fwd' / 'rev' (one FP32 addition per product) or 'mfma'
    (the 32 products of one instruction summed exactly, then rounded into the accumulator).  line / three_terms /
    finite_range: the rule's constants, for the tests that show a weaker rule is caught."""
    M = len(w)
    Wh, Wl, cf, nw, nc = hard_prep(w, mu, var, finite_range)
    nwmax, ncmax = F32(np.fmax.reduce(nw)), F32(np.fmax.reduce(nc))            # (fmaxf: a NaN margin is passed over)
    if finite_range and not nwmax < HARD_FINITE:
        ncmax = F32(np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        z = np.concatenate([X * X, X], axis=1)
        zh, zl = _split_nonfinite(z)
        nxe = (np.sqrt((z * z).sum(1)) * (1.0 + 2.0 ** -20)).astype(F32)
        pairs = [(Wh, zh), (Wh, zl)] + ([(Wl, zh)] if three_terms else [])
        P = np.concatenate([b[:, None, :] * a[None] for a, b in pairs], axis=2).astype(F32)      # exact in float32
        acc = np.repeat(cf[None], len(X), axis=0)
        K = P.shape[2]
        if order == "mfma":
            for k0 in range(0, K, 32):
                acc = (acc.astype(np.float64) + P[:, :, k0:k0 + 32].astype(np.float64).sum(2)).astype(F32)
        else:
            for k in (range(K) if order == "fwd" else reversed(range(K))):
                acc = (acc + P[:, :, k]).astype(F32)
        # the two largest l^ as the kernel keeps them (a NaN neither leads nor comes second)
        b1 = np.full(len(X), -np.inf, F32)
        b2, bm = b1.copy(), np.zeros(len(X), np.int64)
        for m in range(acc.shape[1]):
            v = acc[:, m]
            nb = v > b1
            b2 = np.where(nb, b1, np.fmax(b2, v))
            bm = np.where(nb, m, bm)
            b1 = np.where(nb, v, b1)
        E = ((nwmax * nxe).astype(F32) + ncmax).astype(F32) * F32(1.000001)
        blo, hi2 = (b1 - E).astype(F32), (b2 + E).astype(F32)
        hard = (bm < M) & (blo > F32(-1e29)) & (hi2 < (blo - F32(line)).astype(F32))
        if finite_range:
            hard &= E < HARD_FINITE
    return np.where(hard, bm, M)


def true_logdens(w, mu, var, X, dtype=np.longdouble):
    w, mu, var, X = (np.asarray(a, dtype=dtype) for a in (w, mu, var, X))
    with np.errstate(divide="ignore"):
        base = np.log(w) - 0.5 * (mu.shape[1] * np.log(dtype(2) * dtype(np.pi)) + np.log(var).sum(1))
    return base[None] - 0.5 * (((X[:, None, :] - mu[None]) ** 2) / var[None]).sum(2)


def _mp_gap(w, mu, var, x, owner):
    """true gap of one frame to 60 digits: l_owner minus the best other mixture"""
    import mpmath as mp
    mp.mp.dps = 60
    ls = []
    for m in range(len(w)):
        if w[m] == 0:
            ls.append(-mp.inf)
            continue
        s = mp.log(mp.mpf(w[m])) - mp.mpf(len(x)) / 2 * mp.log(2 * mp.pi)
        for d in range(len(x)):
            v = mp.mpf(var[m, d])
            s -= mp.log(v) / 2 + (mp.mpf(x[d]) - mp.mpf(mu[m, d])) ** 2 / (2 * v)
        ls.append(s)
    return ls[owner] - max(l for k, l in enumerate(ls) if k != owner)


GAPS = (0.0, 1.0, 20.0, 36.0, 300.0, 690.0, 700.0, 720.0, 740.0, 744.0, 745.0, 745.3, 745.6, 746.0, 746.5, 748.0, 752.0, 760.0,
        800.0, 1e3, 1e4, 1e5, 1e6)


def _frames_at_gaps(rng, w, mu, var, npairs):
    """frames on segments x_p -> mu_q with l_p - l_q bisected to each of GAPS (plus draws of the model): the frames the 746-nat
    line is about"""
    M, dj = mu.shape
    live = np.flatnonzero(w > 0)
    p = rng.choice(live, npairs)
    q = np.array([rng.choice(live[live != a]) for a in p])
    Xp = mu[p] + 0.5 * rng.standard_normal((npairs, dj)) * np.sqrt(var[p])
    seg = lambda s: Xp + s[:, None] * (mu[q] - Xp)                        # noqa: E731

    def gap(s):
        L = true_logdens(w, mu, var, seg(s), np.float64)
        return L[np.arange(npairs), p] - L[np.arange(npairs), q]
    out = [mu[rng.choice(live, 4 * npairs)] + rng.standard_normal((4 * npairs, dj)) * np.sqrt(var[rng.choice(live, 4 * npairs)])]
    for g in GAPS:
        lo, hi = np.zeros(npairs), np.ones(npairs)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            ok = gap(mid) >= g
            lo, hi = np.where(ok, mid, lo), np.where(ok, hi, mid)
        out.append(seg(lo))
    return np.concatenate(out)


def _check_hard_keys(w, mu, var, X, **rule):
    """every frame declared hard, in every summation order: true gap > 745.2 nats and the true arg-max; returns the number of
    hard frames"""
    L = true_logdens(w, mu, var, X)
    top = np.argmax(L, axis=1)
    Ls = np.sort(L, axis=1)
    gap = Ls[:, -1] - Ls[:, -2]
    nhard = 0
    for order in ("fwd", "rev", "mfma"):
        k = hard_keys(w, mu, var, X, order, **rule)
        h = np.flatnonzero(k < len(w))
        nhard += len(h)
        wrong = h[k[h] != top[h]]
        assert len(wrong) == 0, f"{order}: frames {wrong[:5]} certified hard to {k[wrong[:5]]}, true owners {top[wrong[:5]]} (gaps {gap[wrong[:5]]})"
        short = h[gap[h] <= 745.2]
        assert len(short) == 0, f"{order}: frames {short[:5]} certified hard at true gaps {gap[short[:5]]}"
        for f in h[gap[h] < 750.0][:8]:                                   # the frames nearest the line, once more to 60 digits
            assert _mp_gap(w, mu, var, X[f], int(k[f])) > 745.2
    return nhard


def _model(rng, M, dj, sep, vlo, vhi, shift=0.0, zero=()):
    w = rng.dirichlet(2.0 * np.ones(M))
    w[list(zero)] = 0.0
    w /= w.sum()
    var = np.exp(rng.uniform(np.log(vlo), np.log(vhi), (M, dj)))
    mu = sep * rng.standard_normal((M, dj)) + shift
    return w, mu, var


HARD_MODELS = {
    # name: (M, dj, sep, var lo, var hi, shift, zero-weight mixtures)
    "random": (40, 24, 6.0, 0.05, 1.0, 0.0, ()),
    "tight": (37, 48, 10.0, 1e-7, 1e-2, 0.0, ()),
    # (margins of 1e6 .. 1e8 nats: no frame settles -- the check is that none is settled wrongly)
    "shift+300": (24, 16, 20.0, 0.05, 1.0, 300.0, ()),
    "shift-2000": (24, 16, 20.0, 0.05, 1.0, -2000.0, ()),
    "zero-weight": (33, 32, 6.0, 0.05, 1.0, 0.0, (0, 7, 32)),
    "M17": (17, 80, 2.0, 0.1, 1.0, 0.0, (16,)),
}


@pytest.mark.parametrize("name", sorted(HARD_MODELS))
def test_hard_key_is_sound(name):
    M, dj, sep, vlo, vhi, shift, zero = HARD_MODELS[name]
    rng = np.random.default_rng(sorted(HARD_MODELS).index(name))
    w, mu, var = _model(rng, M, dj, sep, vlo, vhi, shift, zero)
    X = _frames_at_gaps(rng, w, mu, var, 24)
    nhard = _check_hard_keys(w, mu, var, X)
    if shift == 0.0:                                 # (the screen does settle frames here: the check is not vacuous)
        assert nhard > 0.05 * 3 * len(X), nhard / (3 * len(X))


def _one_dominant_term_cases(n, seed):
    """M = 2, one dimension: two mixtures centred at 0 with variances v and r v (r = 1.05 .. 1.3), frames on the axis with
    l_p - l_q bisected to within 30 nats either side of 745.2.  |W z| is ~10x the gap and dominated by ONE product, so a rounding
    error of the operands is as large against the margin E as it gets -- the case a weaker rule fails first."""
    rng = np.random.default_rng(seed)
    gaps = np.r_[745.2 - np.r_[0.0, np.geomspace(0.01, 30, 30)], 745.2 + np.geomspace(0.01, 30, 30)]
    for _ in range(n):
        v, r = np.exp(rng.uniform(np.log(1e-3), np.log(1e-1))), rng.uniform(1.05, 1.3)
        w, mu, var = np.array([0.5, 0.5]), np.zeros((2, 2)), np.ones((2, 2))
        var[0, 0], var[1, 0] = r * v, v
        lo, hi = np.zeros(len(gaps)), np.full(len(gaps), 1e4)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            L = true_logdens(w, mu, var, np.c_[mid, np.zeros_like(mid)], np.float64)
            ok = L[:, 0] - L[:, 1] <= gaps
            lo, hi = np.where(ok, mid, lo), np.where(ok, hi, mid)
        yield w, mu, var, np.c_[lo, np.zeros_like(lo)]


def test_hard_key_next_to_the_line():
    nhard = sum(_check_hard_keys(w, mu, var, X) for w, mu, var, X in _one_dominant_term_cases(60, 11))
    assert nhard > 1000, nhard


def _overflow_models():
    """models whose operands leave the float32 range: -1/(2 var) below -FLT_MAX (var < ~1.5e-39) or mu / var beyond it, with
    frames that such a mixture owns -- small |x|, so that the margin E of the frame stays finite"""
    yield (np.array([0.5, 0.5]), np.array([[1e-8, 0.0], [0.0, 0.0]]), np.array([[1e-39, 1.0], [1.0, 1.0]])), np.array([[1e-8, 0.0]])
    rng = np.random.default_rng(5)
    for vt, mt in ((1e-39, 1e-9), (1e-41, 0.0), (1e-36, 1e-2)):
        M, dj = 20, 8
        w, mu, var = _model(rng, M, dj, 1e-3, 0.5, 1.0)
        var[:3, 0] = vt                                       # three mixtures with one tight dimension
        mu[:3, 0] = mt
        X = np.concatenate([mu[:3] + 1e-9 * rng.standard_normal((3, dj)) * np.r_[0.0, np.ones(dj - 1)],
                            mu[rng.choice(M, 64)] + 1e-3 * rng.standard_normal((64, dj))])
        X[:3, 0] = mt
        yield (w, mu, var), X


def test_hard_key_on_models_beyond_the_float_range():
    """a mixture whose operands overflow FP32 has a NaN or -inf l^; without kHardFinite it drops out of the comparison and the
    frames it owns could be certified hard to another mixture -- with it they are left soft"""
    for (w, mu, var), X in _overflow_models():
        _check_hard_keys(w, mu, var, X)
