"""adversarial.py -- frames on which a wrong screen-out WOULD show (VERDICT r5 "Next round" item 1).  TEST INFRASTRUCTURE ONLY:
imported by tests/ and __graft_entry__.smoke(); drives the C oracle (vco_logdens = lpr of src/gmm.jl:25-27) to PLACE the frames.

The frames a model's own p(x) produces have, on a peaked model (eigenvalues down to 1e-5), one live mixture each:
every screening decision is far from its threshold.  The kernels that skip work on a proof (csrc/gmmmap_screen.hpp: fvconvert
shape 3 with the FP64 or the bf16-split screen; gmmmap_screen_argmax_kernel) are wrong exactly where they rule out a mixture
that carries posterior mass, so the frames built here put posterior mass where p(x) never does:

  tie        for a pair (a, b): x_a ~ N_a, x_b ~ N_b; the point of the segment x_a -> x_b where mixture a stops being the
             arg-max (bisection on the oracle's arg-max): a and the mixture that takes over have EQUAL log-weighted density
             there and share the posterior -- on a peaked model as well.
  seg        the point of the segment mu_a -> mu_b where lpr_a = lpr_b (whatever a third mixture does there).
  imb        along the same x_a -> x_b segments, the points where a leads / trails the best other mixture by 1, 20, 45 and 47 nats:
             either side of one posterior share, and either side of the e^-46 line below which fvconvert drops a term
             (vcmi_gmmmap_set_prune, default 46).
  triple     a boundary point a | b slid along the boundary until the mixture that takes over changes: three (nearly) equal
             log-densities (nested bisection; kept when the top three lie within `triple_tol` nats).
  outlier    mu_m + r L_m z for r = 1e2, 1e3, 1e4 ("sigmas"), and ordinary frames shifted by +-2000 in every feature: the
             bf16 screen's certified margin eps = 2^-12 (|P||x| + |c|) is largest there.

adversarial_frames() returns the frames, a category code per frame and, from the oracle, the gap between the best and the second
best log-density at each (what the tests use to know which arg-max decisions rounding may legitimately flip).
"""
import numpy as np

CATEGORIES = ("tie", "seg", "imb", "triple", "outlier", "shift")
IMBALANCES = (1.0, 20.0, 45.0, 47.0)


def _chol_x(sig, D):
    return [np.linalg.cholesky((s[:D, :D] + s[:D, :D].T) / 2.0) for s in sig]


def _top2(L):
    """(arg-max, best, second best) per row of the (n, M) log-density matrix"""
    top = np.argmax(L, axis=1)
    best = L[np.arange(len(L)), top]
    L2 = L.copy()
    L2[np.arange(len(L)), top] = -np.inf
    return top, best, np.max(L2, axis=1)


def _lead(L, a):
    """lpr_a - max_{c != a} lpr_c per row"""
    n = np.arange(len(L))
    la = L[n, a]
    L2 = L.copy()
    L2[n, a] = -np.inf
    return la - np.max(L2, axis=1)


def _bisect(pred, lo, hi, iters):
    """largest s (to 2^-iters of the bracket) with pred(s) true, given pred(lo) true and pred(hi) false, vectorised"""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        ok = pred(mid)
        lo = np.where(ok, mid, lo)
        hi = np.where(ok, hi, mid)
    return lo, hi


def adversarial_frames(ref, w, mu, sig, D, seed, npairs=2016, nimb=500, ntriples=150, noutliers=192, triple_tol=1e-3):
    """ref: oracle.c_oracle.GMMMap of (w, mu, sig); returns dict(X (n, D), cat (n,) index into CATEGORIES, pair (n, 2))."""
    rng = np.random.default_rng(seed)
    M = len(w)
    live = np.flatnonzero(np.asarray(w) > 0.0)
    Ls = _chol_x(sig, D)
    mux = np.asarray(mu)[:, :D]

    def draw(m):
        return mux[m] + rng.standard_normal(D) @ Ls[m].T

    # ordered pairs of live mixtures, every unordered pair once while they last, then random ones
    allp = [(a, b) for i, a in enumerate(live) for b in live[i + 1:]]
    rng.shuffle(allp)
    while len(allp) < npairs:
        a, b = rng.choice(live, 2, replace=False)
        allp.append((int(a), int(b)))
    pairs = np.array(allp[:npairs], dtype=np.int64)
    a_idx, b_idx = pairs[:, 0], pairs[:, 1]
    Xa = np.stack([draw(a) for a in a_idx])
    Xb = np.stack([draw(b) for b in b_idx])
    seg = lambda s, P0=Xa, P1=Xb: P0 + s[:, None] * (P1 - P0)          # noqa: E731

    out_X, out_cat, out_pair = [], [], []

    def emit(X, cat, pr):
        out_X.append(np.atleast_2d(X))
        out_cat.append(np.full(len(np.atleast_2d(X)), CATEGORIES.index(cat), dtype=np.int64))
        out_pair.append(np.atleast_2d(pr))

    # ---- tie: where a stops being the arg-max on x_a -> x_b
    a_top = lambda s: np.argmax(ref.logdens(seg(s)), axis=1) == a_idx    # noqa: E731
    ok0 = a_top(np.zeros(npairs)) & ~a_top(np.ones(npairs))              # (a draw of a whose arg-max is not a: dropped)
    lo, hi = _bisect(lambda s: a_top(s) | ~ok0, np.zeros(npairs), np.ones(npairs), 58)
    s0 = lo
    emit(seg(lo)[ok0], "tie", pairs[ok0])
    emit(seg(hi)[ok0], "tie", pairs[ok0])                                  # ... and the first point on the other side

    # ---- imb: a leads / trails the best other mixture by d nats, on the first `nimb` segments
    k = min(nimb, npairs)
    sub = np.arange(k)
    lead = lambda s: _lead(ref.logdens(Xa[sub] + s[:, None] * (Xb[sub] - Xa[sub])), a_idx[sub])     # noqa: E731
    for d in IMBALANCES:
        lo_p, _ = _bisect(lambda s: lead(s) >= d, np.zeros(k), s0[sub], 36)                          # a ahead by d
        _, hi_m = _bisect(lambda s: lead(s) >= -d, s0[sub], np.ones(k), 36)                          # a behind by d
        keep = ok0[sub]
        emit((Xa[sub] + lo_p[:, None] * (Xb[sub] - Xa[sub]))[keep], "imb", pairs[sub][keep])
        emit((Xa[sub] + hi_m[:, None] * (Xb[sub] - Xa[sub]))[keep], "imb", pairs[sub][keep])

    # ---- seg: lpr_a = lpr_b on mu_a -> mu_b (the verdict's literal construction)
    Ma, Mb = mux[a_idx], mux[b_idx]
    n = np.arange(npairs)

    def a_over_b(s):
        L = ref.logdens(Ma + s[:, None] * (Mb - Ma))
        return L[n, a_idx] >= L[n, b_idx]
    lo, _ = _bisect(a_over_b, np.zeros(npairs), np.ones(npairs), 58)
    emit(Ma + lo[:, None] * (Mb - Ma), "seg", pairs)

    # ---- triple: slide the a | . boundary point from x_b towards x_c until the mixture that takes over changes
    if ntriples > 0 and len(live) >= 3:
        tri = np.array([rng.choice(live, 3, replace=False) for _ in range(ntriples)], dtype=np.int64)
        Ta = np.stack([draw(m) for m in tri[:, 0]])
        Tb = np.stack([draw(m) for m in tri[:, 1]])
        Tc = np.stack([draw(m) for m in tri[:, 2]])
        ta = tri[:, 0]

        nt = ntriples

        def boundary(v):
            """v: (nt, G) end-point parameters -> the a-side boundary points on x_a -> x_b + v (x_c - x_b), (nt, G, D), and the
            mixture on their other side (nt, G); all nt * G segments bisected in one batch (one oracle call per step)"""
            G = v.shape[1]
            End = (Tb[:, None, :] + v[:, :, None] * (Tc - Tb)[:, None, :]).reshape(nt * G, D)
            Sta = np.repeat(Ta, G, axis=0)
            aa = np.repeat(ta, G)
            top_a = lambda s: np.argmax(ref.logdens(Sta + s[:, None] * (End - Sta)), axis=1) == aa          # noqa: E731
            lo_s, hi_s = _bisect(top_a, np.zeros(nt * G), np.ones(nt * G), 44)
            other = np.argmax(ref.logdens(Sta + hi_s[:, None] * (End - Sta)), axis=1)
            return (Sta + lo_s[:, None] * (End - Sta)).reshape(nt, G, D), other.reshape(nt, G)
        # the mixture that takes over at v = 0 and at v = 1; where they differ, narrow the v at which it changes on a grid of G
        # points per level (G^levels ~ 1e9: as fine as 30 bisection steps, in a tenth of the oracle calls)
        G, levels = 8, 10
        _, oe = boundary(np.stack([np.zeros(nt), np.ones(nt)], axis=1))
        o0, o1 = oe[:, 0], oe[:, 1]
        cand = (o0 != o1) & (o0 != ta) & (o1 != ta)
        vlo, vhi = np.zeros(nt), np.ones(nt)
        for _ in range(levels):
            grid = vlo[:, None] + (vhi - vlo)[:, None] * (np.arange(1, G + 1) / (G + 1.0))[None, :]
            _, og = boundary(grid)
            same = og == o0[:, None]                                   # (nt, G): still the v = 0 mixture on the other side
            first = np.where(same.all(axis=1), G, np.argmin(same, axis=1))          # first grid point where it is not
            allg = np.concatenate([vlo[:, None], grid, vhi[:, None]], axis=1)      # (nt, G + 2)
            vlo, vhi = allg[np.arange(nt), first], allg[np.arange(nt), first + 1]
        P = boundary(vlo[:, None])[0][:, 0, :]
        Lp = np.sort(ref.logdens(P), axis=1)
        good = cand & (Lp[:, -1] - Lp[:, -3] < triple_tol)
        emit(P[good], "triple", tri[good][:, :2])

    # ---- outliers and shifted frames
    per = max(noutliers // 3, 1)
    for r in (1e2, 1e3, 1e4):
        ms = rng.choice(live, per)
        emit(np.stack([mux[m] + r * (rng.standard_normal(D) @ Ls[m].T) for m in ms]), "outlier", np.stack([ms, ms], 1))
    ms = rng.choice(live, per)
    base = np.stack([draw(m) for m in ms])
    emit(base + 2000.0, "shift", np.stack([ms, ms], 1))
    emit(base - 2000.0, "shift", np.stack([ms, ms], 1))

    X = np.ascontiguousarray(np.concatenate(out_X))
    return {"X": X, "cat": np.concatenate(out_cat), "pair": np.concatenate(out_pair)}


def mixed_call(ref, w, mu, sig, D, seed, ratio=9, min_frames=8192, **kw):
    """The adversarial frames scattered 1 : ratio among draws from the model's own p(x) (at least `min_frames` in all, so that the
    call is grouped and takes the screened kernels).  Returns (X (T, D), is_adversarial (T,), cat (T,) with -1 for p(x) draws,
    gap (T,): best minus second best oracle log-density)."""
    import synthdata
    adv = adversarial_frames(ref, w, mu, sig, D, seed, **kw)
    na = len(adv["X"])
    nplain = max(ratio * na, min_frames - na)
    Xp = synthdata.sample_frames(seed + 1, np.asarray(w), np.asarray(mu), np.asarray(sig), nplain, 0, D)
    X = np.concatenate([adv["X"], Xp])
    cat = np.concatenate([adv["cat"], np.full(nplain, -1, dtype=np.int64)])
    order = np.random.default_rng(seed + 2).permutation(len(X))
    X, cat = np.ascontiguousarray(X[order]), cat[order]
    _, best, second = _top2(ref.logdens(X))
    return X, cat >= 0, cat, best - second


# ------------------------------------------------------------------------------------------------ E-step (diagonal / full)
# The E-step kernels (csrc/estep_hard.hpp, estep.hip, estep_small.hpp, estep_wave.hpp) skip work or switch formulas where a
# log-density crosses a line: 36 nats (kRefine: term-by-term re-evaluation), 745.2 (VCMI_ESTEP_EXP_SKIP, and where exp
# underflows), 746 (the hard key).  estep_sentinel_call() builds calls whose frames sit on those lines and makes each decision
# visible in the statistics of ONE mixture:
#   background  far-apart mixtures owning the model's p(x) draws (>= 65,536 frames: the hard-assignment path is in play); mixture
#               0 has 100x wider variances than the rest and owns the outliers and the shifted frames; mixture 1 has weight 0
#               and sits 3 sigma from mixture 0 (frames whose nearest mixture has no weight);
#   sentinels   one per gap class g, each a copy of its owner's variances and weight at 60 sigma along its own direction
#               (orthonormal per owner): the class's frames lie on x_p -> mu_q with l_p - l_q bisected to g, and nothing else in
#               the call comes within ~1000 nats of the sentinel -- its S0, S1, S2 are made of the responsibilities under test;
#   triple      two sentinels q, r of one owner and a frame equidistant from all three (equal weights and variances);
#   outliers    mu_0 + r sigma_0 z for r = 1e2, 1e3, 1e4 (every l ~ -1e8: the expanded form is off by ~1e-6, the refinement
#               must fire) and draws of mixture 0 shifted by +-2000.
ESTEP_GAPS = (0.0, 1.0, 20.0, 35.5, 36.5, 45.0, 300.0, 690.0, 744.0, 745.5, 746.5, 760.0)
_SENT_SIGMAS = 60.0


def estep_logdens(X, w, mu, var, dtype=np.longdouble):
    """vco_estep_diag's log-densities, term by term, in `dtype` (frames (n, Dj), parameters [m][d]) -> (n, M)"""
    w, mu, var, X = (np.asarray(a, dtype=dtype) for a in (w, mu, var, X))
    with np.errstate(divide="ignore"):
        cst = np.log(w) - 0.5 * (mu.shape[1] * np.log(dtype(2) * dtype(np.pi)) + np.log(var).sum(1))
    out = np.empty((len(X), len(w)), dtype=dtype)
    for i in range(0, len(X), 4096):
        x = X[i:i + 4096]
        out[i:i + 4096] = cst[None] - 0.5 * (((x[:, None, :] - mu[None]) ** 2) / var[None]).sum(2)
    return out


def estep_sentinel_call(Dj, M, seed, tight=False, nbg=65_536, per_class=8, ratio=9, base=None):
    """-> dict(w, mu, var ([m][d]), X (N, Dj), cls (N,) -1 = p(x) draw / index into ESTEP_GAPS / len(ESTEP_GAPS) = triple /
    len + 1 = outlier or shifted frame, sent (len(ESTEP_GAPS) + 1,) the sentinel of each class (the triple: its first one),
    owner (same), gap (N,) the achieved l_owner - l_sentinel).  tight: variances 1e-7 .. 1e-2 and means ~10 (the refinement's
    regime).  base: (w, mu, var) of the background (a trained model) instead of synthetic mixtures.  M counts every mixture;
    classes that do not fit (M too small) are left out, from the triple on, then from the largest gap down."""
    rng = np.random.default_rng(seed)
    ncls = len(ESTEP_GAPS)
    if base is not None:
        bw, bmu, bvar = (np.array(a, dtype=np.float64) for a in base)
        nb = len(bw)
    else:
        nb = max(3, M - ncls - 2)
        lo, hi = (1e-7, 1e-2) if tight else (0.05, 1.0)
        bvar = np.exp(rng.uniform(np.log(lo), np.log(hi), (nb, Dj)))
        bmu = (10.0 if tight else 0.0) + np.sqrt(bvar.max()) * 40.0 * rng.standard_normal((nb, Dj))
        bw = rng.dirichlet(4.0 * np.ones(nb))
        bvar[0] = 100.0 * bvar[0]                               # the wide mixture
        bw[1] = 0.0                                             # the weightless one, 3 sigma from the wide one
        bmu[1] = bmu[0] + 3.0 * np.sqrt(bvar[0]) * rng.choice([-1.0, 1.0], Dj)
        bw /= bw.sum()
    room = M - nb
    gaps = list(ESTEP_GAPS)
    triple = room >= ncls + 2
    while len(gaps) > room - (2 if triple else 0):
        gaps.pop()
    assert gaps, "no room for sentinels"
    owners = [m for m in range(2 if base is None else 0, nb) if bw[m] > 0]
    owners = [owners[i % len(owners)] for i in range(len(gaps) + (1 if triple else 0))]
    w, mu, var = np.zeros(M), np.zeros((M, Dj)), np.ones((M, Dj))
    w[:nb], mu[:nb], var[:nb] = bw, bmu, bvar
    # sentinel directions: orthonormal per owner, in the owner's own metric (so ties are exact when var and w are copied)
    dirs = {}
    for p in set(owners):
        k = owners.count(p) + 1
        dirs[p] = list(np.linalg.qr(rng.standard_normal((Dj, k)))[0].T)
    sent, q = [], nb
    for p in owners:
        sent.append(q)
        u = dirs[p].pop()
        w[q], var[q] = w[p], var[p]
        # (offset and means on a grid of 2^-24: the mid-point of the tie class is exact, x - mu_p = mu_q - x)
        mu[p] = np.ldexp(np.round(np.ldexp(mu[p], 24)), -24)
        mu[q] = mu[p] + 2.0 * np.ldexp(np.round(np.ldexp(0.5 * _SENT_SIGMAS * np.sqrt(var[p]) * u, 24)), -24)
        q += 1
    if triple:
        p = owners[-1]
        u = dirs[p].pop()
        w[q], var[q] = w[p], var[p]
        mu[q] = mu[p] + _SENT_SIGMAS * np.sqrt(var[p]) * u
        q += 1
    Mu = q
    w[Mu:] = 0.0                                                # (unused slots: weightless copies of mixture 0 far away)
    mu[Mu:] = mu[0] + 1e3 * np.sqrt(var[0])
    var[Mu:] = var[0]
    # background draws
    comp = rng.choice(nb, size=nbg, p=bw)
    Xb = mu[comp] + rng.standard_normal((nbg, Dj)) * np.sqrt(var[comp])
    Xs, cls, gap_out = [], [], []
    for k, g in enumerate(gaps):
        p, s = owners[k], sent[k]
        if g == 0.0:                                            # exact tie: the mid-point of the means
            X = np.repeat((0.5 * (mu[p] + mu[s]))[None], per_class, 0)
            X[1:] += 1e-3 * np.sqrt(var[p]) * rng.standard_normal((per_class - 1, Dj)) * (mu[s] - mu[p] == 0)
        else:
            x0 = mu[p] + 0.5 * np.sqrt(var[p]) * rng.standard_normal((per_class, Dj))
            seg = lambda t, x0=x0, s=s: x0 + t[:, None] * (mu[s] - x0)                     # noqa: E731

            def pred(t, p=p, s=s, g=g, seg=seg):
                L = estep_logdens(seg(t), w[[p, s]], mu[[p, s]], var[[p, s]])
                return L[:, 0] - L[:, 1] >= g
            t, _ = _bisect(pred, np.zeros(per_class), np.ones(per_class), 64)
            X = seg(t)
        L = estep_logdens(X, w[[p, s]], mu[[p, s]], var[[p, s]])
        Xs.append(X)
        cls.append(np.full(len(X), k))
        gap_out.append(np.asarray(L[:, 0] - L[:, 1], dtype=np.float64))
    if triple:
        p, a, b = owners[-1], sent[-1], Mu - 1
        # x = mu_p + alpha da + beta db equidistant from the three in the metric 1/var: two linear equations
        S = np.sqrt(var[p])
        da, db = (mu[a] - mu[p]) / S, (mu[b] - mu[p]) / S
        G = np.array([[da @ da, da @ db], [da @ db, db @ db]])
        al, be = np.linalg.solve(2.0 * G, np.array([da @ da, db @ db]))
        X = np.repeat((mu[p] + S * (al * da + be * db))[None], per_class, 0)
        Xs.append(X)
        cls.append(np.full(per_class, ncls))
        L = estep_logdens(X, w[[p, a]], mu[[p, a]], var[[p, a]])
        gap_out.append(np.asarray(L[:, 0] - L[:, 1], dtype=np.float64))
    # outliers and shifted frames (mixture 0 owns them)
    per = max(per_class, 4)
    Xo = [mu[0] + r * np.sqrt(var[0]) * rng.standard_normal((per, Dj)) / np.sqrt(Dj) for r in (1e2, 1e3, 1e4)]
    d0 = mu[0] + rng.standard_normal((2 * per, Dj)) * np.sqrt(var[0])
    Xo += [d0[:per] + 2000.0, d0[per:] - 2000.0, mu[1] + 0.1 * np.sqrt(var[0]) * rng.standard_normal((per, Dj))]
    if base is None:
        Xs += Xo
        cls += [np.full(len(x), ncls + 1) for x in Xo]
        gap_out += [np.full(len(x), np.nan) for x in Xo]
    Xa = np.concatenate(Xs)
    ca = np.concatenate(cls)
    ga = np.concatenate(gap_out)
    # the adversarial frames scattered among the p(x) draws, in a fixed random order
    n = len(Xa)
    pos = np.sort(rng.choice(nbg + n, n, replace=False))
    X = np.empty((nbg + n, Dj))
    c = np.full(nbg + n, -1)
    gg = np.full(nbg + n, np.nan)
    mask = np.zeros(nbg + n, bool)
    mask[pos] = True
    perm = rng.permutation(n)
    X[mask], c[mask], gg[mask] = Xa[perm], ca[perm], ga[perm]
    X[~mask] = Xb
    return dict(w=w, mu=mu, var=var, X=np.ascontiguousarray(X), cls=c, gap=gg, sent=np.array(sent), owner=np.array(owners),
                gaps=np.array(gaps), Mu=Mu, nb=nb)


# ---------------------------------------------------------------------------------------------------------------
# Frames on the silence threshold of align_mcep (src/align.jl:47-52: keep a frame when log mc2e(src) > threshold)
# ---------------------------------------------------------------------------------------------------------------
def frames_at_energy_threshold(mc, alpha, fftlen, threshold, gaps):
    """Moves every frame of mc (T,D) so that its log-energy lies `gaps[i]` above (positive) or below (negative) `threshold`.

    A constant term is invariant under frequency warping, so adding a to c0 multiplies the impulse response by e^a and adds
    exactly 2a to log mc2e: one step  c0 += (threshold + gap - log e) / 2  lands on the requested gap up to the rounding of
    c0 and of the oracle's own evaluation.  The energies come from the C oracle only (the kernel under test is not asked).
    Returns (mc' (T,D), achieved gaps (T,)) with the achieved gaps re-evaluated by the oracle on mc'."""
    from . import c_oracle as co
    mc = np.array(mc, dtype=np.float64, order="C")
    gaps = np.resize(np.asarray(gaps, dtype=np.float64), len(mc))
    mc[:, 0] += (threshold + gaps - np.log(co.mc2e(mc, alpha, fftlen))) / 2.0
    return mc, np.log(co.mc2e(mc, alpha, fftlen)) - threshold
