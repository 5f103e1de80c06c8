"""GPU parity of the diagonal and full-covariance E-step on frames AT its decision lines (oracle/adversarial.py,
estep_sentinel_call): every kernel skips work or switches formulas where an approximate log-density crosses 36 nats (kRefine),
745.2 (VCMI_ESTEP_EXP_SKIP, the FP64 underflow of exp) or 746 (the hard key of csrc/estep_hard.hpp), and the path of a call
is chosen from a sample of 16 chunks (estep_path.hpp).  Each gap class's frames are the only mass of one SENTINEL mixture, and
the statistics are checked PER MIXTURE (per_mixture_err): a mixture that holds 1e-20 of the data is held to the same relative
accuracy as the largest one -- the M-step divides its S1 and S2 by its own S0 (estep.py mstep_diag / mstep_full).

The contract (include/vcmi.h, vcmi_estep_diag):
  ordinary models   per-mixture relative error <= 1e-9 for every gap class up to 690 nats; 744 .. 746 nats: absolute 1e-320
                    (subnormal responsibilities); >= 746.5 nats: S0 exactly 0, as in the oracle;
  tight variances   per-mixture relative error <= 1e-9 below 36 nats; beyond, each frame's contribution within e^-36 of its
                    own weight;
  every call        log-likelihood to 1e-9 relative, repeat runs bit-identical, AUTO bit-identical to a pinned HARD whenever
                    it takes the hard-assignment path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-9
SUBNORMAL = 1e-320


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def per_mixture_err(got, ref):
    """(S0, S1, S2) against (S0, S1, S2) -- S1 / S2 as (Dj, M) or (Dj, Dj, M) -> (M,): for every mixture the largest error among
    S0[m], S1[..., m] and S2[..., m], each relative to that mixture's own largest reference value (absolute below 1e-300)"""
    out = np.zeros(len(ref[0]))
    for g, r in zip(got, ref):
        g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
        g, r = g.reshape(-1, g.shape[-1]), r.reshape(-1, r.shape[-1])
        den = np.max(np.abs(r), axis=0)
        num = np.max(np.abs(g - r), axis=0)
        out = np.maximum(out, np.where(den < 1e-300, num, num / np.where(den < 1e-300, 1.0, den)))
    return out


def per_mixture_abs(got, ref):
    out = np.zeros(len(ref[0]))
    for g, r in zip(got, ref):
        g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
        out = np.maximum(out, np.max(np.abs(g - r).reshape(-1, len(out)), axis=0))
    return out


_CASES = {}


def _case(Dj, M, tight=False, joint=None, shrink=1.0, seed=0):
    """model + sentinel call + oracle statistics, built once per module"""
    key = (Dj, M, tight, joint is not None, shrink, seed)
    if key not in _CASES:
        from oracle import adversarial as adv, c_oracle as co
        base = None
        if joint is not None:
            w, mu, sig = joint
            base = (w, mu, np.stack([np.diag(s.T).copy() for s in sig]) * shrink)
        c = adv.estep_sentinel_call(Dj, M, 100 + Dj + M + seed, tight=tight, base=base)
        c["ref"] = co.estep_diag(c["X"], c["w"], c["mu"], c["var"])
        _CASES[key] = c
    return _CASES[key]


def _gap_of(c, m):
    """the gap class whose sentinel m is (None: not a sentinel of a gap class)"""
    k = np.flatnonzero(c["sent"][:len(c["gaps"])] == m)
    return float(c["gaps"][k[0]]) if len(k) else None


def _check_contract(c, got, tight, what):
    r0, r1, r2, rl = c["ref"]
    ref = (r0, r1.T, r2.T)
    err = per_mixture_err(got[:3], ref)
    ab = per_mixture_abs(got[:3], ref)
    X = c["X"]
    for m in range(len(r0)):
        g = _gap_of(c, m)
        if g is None or g < (36.0 if tight else 744.0):
            assert err[m] <= TOL, (what, m, g, err[m])
        elif tight:
            n = int(np.sum(c["cls"] == list(c["gaps"]).index(g)))
            xs = np.abs(X[c["cls"] == list(c["gaps"]).index(g)]).max()
            assert ab[m] <= n * np.exp(-36.0) * max(1.0, xs * xs), (what, m, g, ab[m])
        elif g < 746.5:
            assert ab[m] <= SUBNORMAL, (what, m, g, ab[m])
        else:
            assert r0[m] == 0.0 and got[0][m] == 0.0 and not got[1][:, m].any() and not got[2][:, m].any(), (what, m, g, got[0][m])
    assert abs(got[3] - rl) <= TOL * abs(rl), (what, got[3], rl)


def _run(vc, c, path=None, force=0, dev=False):
    from voiceconversion_jl_amd import _lib
    X, w, mu, var = c["X"], c["w"], c["mu"], c["var"]
    if path is not None:
        vc.estep_set_path(path)
    _lib.debug_force(force)
    try:
        if dev:
            import torch
            Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
            st = vc.estep_diag_dev(Xd.t(), w, mu.T, var.T).cpu().numpy()
            S0, S1, S2, ll = vc.unpack_stats(st, X.shape[1], len(w))
            out = (S0.copy(), np.asarray(S1), np.asarray(S2), float(ll))
        else:
            out = vc.estep_diag(X.T, w, mu.T, var.T)
        return out, _lib.estep_last_soft()
    finally:
        _lib.debug_force(0)
        vc.estep_set_path(vc.ESTEP_AUTO)


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]


def test_the_generator_covers_what_it_claims():
    """every gap class is hit to 1e-9 nats, each sentinel's mass is its own class's, and each adversarial frame of a class up to
    690 nats moves its sentinel's statistics by more than the tolerance (dropping it, or zeroing its responsibility, is seen);
    the C oracle agrees with an extended-precision evaluation on the sentinels"""
    from oracle import adversarial as adv
    for Dj, M, tight in ((80, 128, False), (48, 24, False), (80, 128, True)):
        c = _case(Dj, M, tight)
        X, w, mu, var = c["X"], c["w"], c["mu"], c["var"]
        for k, g in enumerate(c["gaps"]):
            got = c["gap"][c["cls"] == k]
            assert len(got) > 0 and np.all(np.abs(got - g) <= 1e-9), (k, g, got)
        assert np.sum(c["cls"] == len(adv.ESTEP_GAPS)) > 0 or M < 40            # triple points where there is room for them
        # responsibilities of the sentinels from every frame, in extended precision
        S = np.asarray(c["sent"])
        L = np.concatenate([adv.estep_logdens(X[i:i + 8192], w, mu, var, np.float64) for i in range(0, len(X), 8192)])
        lse = np.logaddexp.reduce(L, axis=1)
        G = np.exp(L[:, S] - lse[:, None])                                       # (N, sentinels), float64
        idx = np.flatnonzero(c["cls"] >= 0)
        La = adv.estep_logdens(X[idx], w, mu, var)
        mx = La.max(axis=1)
        Ga = np.exp(La - mx[:, None]) / np.exp(La - mx[:, None]).sum(axis=1)[:, None]
        r0, r1, r2, _ = c["ref"]
        for j, (s, g) in enumerate(zip(S, list(c["gaps"]) + [None])):
            own = c["cls"] == (j if g is not None else len(adv.ESTEP_GAPS))
            mine, other = G[own, j].sum(), G[~own, j].sum()
            assert other <= 1e-12 * mine or (mine == 0.0 and other == 0.0), (s, g, mine, other)
            if g is not None and g >= 746.5:
                assert r0[s] == 0.0
                continue
            # the oracle's sentinel statistics against extended precision (744 .. 746: subnormal, absolute)
            sel = c["cls"][idx] == (j if g is not None else len(adv.ESTEP_GAPS))
            e0 = Ga[sel, s].sum()
            e1 = (Ga[sel, s][:, None] * X[idx][sel]).sum(0)
            if g is not None and g >= 744.0:
                assert abs(r0[s] - float(e0)) <= SUBNORMAL
                continue
            assert per_mixture_err((r0[[s]], r1[[s]].T, r2[[s]].T), (np.array([float(e0)]), np.asarray(e1, np.float64)[:, None],
                                   np.asarray((Ga[sel, s][:, None] * X[idx][sel] ** 2).sum(0), np.float64)[:, None]))[0] < 1e-12
            # sensitivity: each frame carries more than the tolerance of its sentinel's S0 and S1
            share = Ga[sel, s] / e0
            s1 = np.abs(Ga[sel, s][:, None] * X[idx][sel]).max(1) / np.abs(e1).max()
            assert share.min() > 100 * TOL and s1.min() > 100 * TOL, (s, g, share.min(), s1.min())


SHAPES = [(80, 128), (48, 24), (80, 16), (50, 17), (80, 160), (79, 40)]


@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("Dj,M", SHAPES)
def test_sentinels_on_every_path(vc, Dj, M, tight):
    """AUTO / HARD / SOFT / the generic kernels / (M <= 32) without the small workgroups, estep_diag and estep_diag_dev: the
    contract on every sentinel, repeat runs bit-identical, AUTO equal to the pinned HARD when it takes that path"""
    from voiceconversion_jl_amd import _lib
    c = _case(Dj, M, tight)
    runs = {"auto": _run(vc, c), "hard": _run(vc, c, vc.ESTEP_HARD), "soft": _run(vc, c, vc.ESTEP_SOFT),
            "generic": _run(vc, c, force=_lib.DBG_ESTEP_GENERIC), "auto_dev": _run(vc, c, dev=True),
            "hard_dev": _run(vc, c, vc.ESTEP_HARD, dev=True)}
    if M <= 32:
        runs["no_small"] = _run(vc, c, force=_lib.DBG_ESTEP_NO_SMALL)
    for name, (got, _) in runs.items():
        _check_contract(c, got, tight, name)
    again = _run(vc, c)
    assert _same(again[0], runs["auto"][0]) and again[1] == runs["auto"][1]
    assert _same(_run(vc, c, vc.ESTEP_HARD)[0], runs["hard"][0])
    assert runs["soft"][1] == -1 and runs["generic"][1] == -1
    if M <= 128:
        assert runs["hard"][1] >= 0
    if runs["auto"][1] >= 0:                       # AUTO took the hard-assignment path: the same bits as pinning it
        assert _same(runs["auto"][0], runs["hard"][0])
        assert _same(runs["auto_dev"][0], runs["hard_dev"][0])


@pytest.mark.parametrize("shrink", [1.0, 1e-3])
def test_sentinels_on_the_reference_model(vc, joint_model, shrink):
    """the reference's trained 32-mixture model (its diagonal) as the background, sentinels added beside it (M = 48)"""
    from voiceconversion_jl_amd import _lib
    c = _case(80, 48, joint=joint_model, shrink=shrink)
    for path, force in ((None, 0), (vc.ESTEP_HARD, 0), (vc.ESTEP_SOFT, 0), (None, _lib.DBG_ESTEP_GENERIC)):
        got, soft = _run(vc, c, path, force)
        _check_contract(c, got, False, (path, force))


def _trap_order(c, owned_first):
    """frames reordered so that the 16 chunks the path decision samples (chunk k * (nchunks // 16) of 1024 frames,
    estep.hip estep_mfma_launch) hold only p(x) draws of one kind and the rest holds the other"""
    from oracle import adversarial as adv
    X = c["X"]
    N = len(X)
    nch = (N + 1023) // 1024
    stride = nch // min(16, nch)
    sampled = np.zeros(N, bool)
    for k in range(min(16, nch)):
        sampled[k * stride * 1024:(k * stride + 1) * 1024] = True
    L = np.concatenate([adv.estep_logdens(X[i:i + 8192], c["w"], c["mu"], c["var"], np.float64) for i in range(0, len(X), 8192)])
    Ls = np.sort(L, axis=1)
    owned = Ls[:, -1] - Ls[:, -2] > 5000.0
    first = np.flatnonzero(owned if owned_first else ~owned)
    rest = np.flatnonzero(~owned if owned_first else owned)
    assert len(first) >= sampled.sum()
    order = np.empty(N, np.int64)
    order[sampled] = first[:sampled.sum()]
    order[~sampled] = np.concatenate([first[sampled.sum():], rest])
    return order


@pytest.mark.parametrize("owned_first", [True, False])
def test_path_decision_traps(vc, owned_first):
    """the sample of 16 chunks holds only owned frames while most of the rest are shared -- or the reverse: the statistics are
    right either way, and estep_last_soft() reports the path taken (0 .. N soft frames: hard-assignment path; -1: one kernel)"""
    from oracle import adversarial as adv, c_oracle as co
    rg = np.random.default_rng(3)
    N, Dj, M = 80_000, 48, 64
    w = rg.dirichlet(4.0 * np.ones(M))
    var = np.exp(rg.uniform(np.log(0.05), 0.0, (M, Dj)))
    mu = 40.0 * rg.standard_normal((M, Dj))
    mu[M // 2:] = mu[M // 2] + 0.3 * rg.standard_normal((M - M // 2, Dj)) * np.sqrt(var[M // 2:])      # overlapping half
    comp = rg.choice(M, size=N, p=w)
    X = mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])
    c = dict(X=X, w=w, mu=mu, var=var)
    X = np.ascontiguousarray(X[_trap_order(c, owned_first)])
    c = dict(X=X, w=w, mu=mu, var=var, ref=co.estep_diag(X, w, mu, var), sent=np.array([], np.int64), gaps=np.array([]),
             cls=np.full(N, -1))
    (got, soft) = _run(vc, c)
    _check_contract(c, got, False, "auto")
    assert (soft >= 0) == owned_first, soft                    # the path follows the sample, whatever the rest holds
    if soft >= 0:
        assert soft > N // 4                                   # ... and the shared frames it did not sample went soft
        assert _same(got, _run(vc, c, vc.ESTEP_HARD)[0])
    assert adv is not None


def test_model_beyond_the_float_range(vc):
    """a mixture with var = 1e-39 in one dimension: -1/(2 var) is -inf in FP32, its bf16-split l^ NaN.  The hard key used to
    let it drop out of the comparison and certify the frames it owns (x ~ 1e-20: the margin E stays finite) as hard to the other
    mixture; now no frame of such a model is hard, and the statistics are the oracle's"""
    from oracle import c_oracle as co
    rg = np.random.default_rng(4)
    N, Dj = 70_000, 16
    w = np.array([0.5, 0.5])
    mu = np.zeros((2, Dj))
    var = np.ones((2, Dj))
    var[0, 0] = 1e-39
    X = rg.standard_normal((N, Dj))
    X[::10] = 1e-20                                            # frames that mixture 0 owns by ~45 nats
    r0, r1, r2, rl = co.estep_diag(X, w, mu, var)
    assert r0[0] > 0.09 * N
    c = dict(X=X, w=w, mu=mu, var=var, ref=(r0, r1, r2, rl), sent=np.array([], np.int64), gaps=np.array([]), cls=np.full(N, -1))
    for path in (vc.ESTEP_HARD, None):
        got, soft = _run(vc, c, path)
        assert per_mixture_err(got[:3], (r0, r1.T, r2.T)).max() <= TOL, (path, per_mixture_err(got[:3], (r0, r1.T, r2.T)))
        assert abs(got[3] - rl) <= TOL * abs(rl)


# ---- full covariance: the same sentinels with full (rotated) covariances, lists on and off ----

def _full_case(Dj, M):
    key = ("full", Dj, M)
    if key not in _CASES:
        from oracle import adversarial as adv, c_oracle as co
        c = adv.estep_sentinel_call(Dj, M, 7 + Dj + M, nbg=4096)
        # full covariances with the same log-densities: sigma = diag(var) exactly (the generator's lines hold) -- plus, for the
        # background mixtures, a rotation (their frames are drawn from diag, but they own them by thousands of nats either way)
        sig = np.stack([np.diag(v) for v in c["var"]])
        rg = np.random.default_rng(1)
        for m in range(c["nb"]):
            Q, _ = np.linalg.qr(rg.standard_normal((Dj, Dj)))
            s = np.sqrt(c["var"][m])
            C = (Q * 0.2) @ Q.T
            np.fill_diagonal(C, 1.0)
            sig[m] = s[:, None] * C * s[None, :]
        c["sig"] = sig
        c["ref"] = co.estep_full(c["X"], c["w"], c["mu"], sig)
        _CASES[key] = c
    return _CASES[key]


@pytest.mark.parametrize("Dj,M", [(24, 32), (40, 20)])
def test_full_covariance_sentinels(vc, Dj, M):
    from conftest import julia_model
    from voiceconversion_jl_amd import _lib
    c = _full_case(Dj, M)
    X = c["X"]
    assert len(X) >= 4096
    r0, r1, r2, rl = c["ref"]
    w, muj, sigj = julia_model(c["w"], c["mu"], c["sig"])
    outs = {}
    for name, force, dev in (("lists", 0, False), ("no_lists", _lib.DBG_ESTEP_FULL_NO_LISTS, False), ("dev", 0, True)):
        _lib.debug_force(force)
        try:
            if dev:
                import torch
                st = vc.estep_full_dev(torch.from_numpy(np.ascontiguousarray(X)).cuda().t(), w, muj, sigj).cpu().numpy()
                S0, S1, S2, ll = vc.unpack_full_stats(st, Dj, M)
                got = (S0.copy(), np.asarray(S1), np.asarray(S2), float(ll))
            else:
                got = vc.estep_full(X.T, w, muj, sigj)
        finally:
            _lib.debug_force(0)
        outs[name] = got
        ref = (r0, r1.T, np.transpose(r2, (1, 2, 0)))
        err = per_mixture_err(got[:3], ref)
        ab = per_mixture_abs(got[:3], ref)
        for m in range(M):
            g = _gap_of(c, m)
            if g is None or g < 744.0:
                assert err[m] <= TOL, (name, m, g, err[m])
            elif g < 746.5:
                assert ab[m] <= SUBNORMAL, (name, m, g, ab[m])
            else:
                assert r0[m] == 0.0 and got[0][m] == 0.0 and not got[1][:, m].any() and not got[2][..., m].any(), (name, m, g)
        assert abs(got[3] - rl) <= TOL * abs(rl)
    assert _same(outs["lists"], vc.estep_full(X.T, w, muj, sigj))
