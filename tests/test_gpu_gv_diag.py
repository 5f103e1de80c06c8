"""GPU: DiagTrajectoryGVGMMMap -- the GV ascent over diagonal conditional precisions (csrc/traj_gv_band.hip: traj_gvd_kernel), over
both converter kinds: a BlockDiagTrajectoryGMMMap ("bdiag") and a TrajectoryGMMMap(precision="diag") ("dense").

The step check is tests/test_gpu_gv_steps.py's: for epoch counts n,

    y_n = fvconvert(tgv, X, epochs=n, alpha),  y_{n+1} = the same call with n + 1      (the n call is repeated: same bits)
    | (y_{n+1} - y_n) - alpha (lik + gv)(y_n) |  <=  bar        element by element,

the gradient from gv_restatement.gradient_terms (imported, unchanged) on the pieces of tests/gv_diag_restatement.py in long double
AT THE DEVICE'S OWN y_n, and

    bar = K 2^-53 ( |y_n| + |y_{n+1}| + alpha (lik_mag + gv_mag) ),     K = 3 * 2D + T + D + 16   (+ 2D in the dense mode),

gv_restatement.step_bar's, fed the magnitude of E in the form the device sums it (gv_diag_restatement's docstring derives both
changes).  The kernel's chain is shorter than the 3 * 2D the bar counts (diag(q) times u is one term): the bar is an upper bound,
not tightened.  At n = 0 eq. (58) has just made var_1(y) = mu_v: the GV term is within its own share of the bar.  Inputs, alpha
and the GV covariance scale per case come from the host (tests/test_gv_diag_restatement_host.py shows both summands visible and
every mutant -- the Gauss-Seidel update among them -- a hundred bars off); odd and even epoch counts are both among n and n + 1:
the parity of the Jacobi buffers decides where the result lands.

Every test here needs DiagTrajectoryGVGMMMap and fails without it."""
import functools

import numpy as np
import pytest

import gv_diag_restatement as gd
import gv_restatement as gr
import traj_bdiag_restatement as tb
from conftest import julia_model
from gv_restatement import EPS, LD

pytestmark = pytest.mark.gpu

KINDS = ("bdiag", "dense")


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def _traj(vc, kind, model, L):
    if kind == "bdiag":
        return vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(*model), L)
    return vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*model)), L, precision="diag")


def _converter(vc, case, L):
    inp = gd.inputs(case)
    return vc.DiagTrajectoryGVGMMMap(_traj(vc, case.kind, inp["model"], L), inp["muv"], np.asfortranarray(inp["Sv"]))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_steps(case, convert, label):
    """convert(n) -> y_n (D,T) of the case's utterance; the step check at every n of case.ns"""
    p = gd.inputs(case)["pieces"]
    D, T, alpha = case.D, case.T, case.alpha
    ys = {n: convert(n) for n in sorted(set(case.ns) | {n + 1 for n in case.ns})}
    K = gd.chain_length(p)
    for n in case.ns:
        assert _same_bits(convert(n), ys[n]), f"{label}: epochs={n} twice gives different bits"
        y_n, y_n1 = np.asarray(ys[n]).T, np.asarray(ys[n + 1]).T
        assert y_n.shape == (T, D) and np.all(np.isfinite(y_n)) and np.all(np.isfinite(y_n1))
        lik, gv, _, gv_mag = gr.gradient_terms(p, y_n)
        bar = gd.step_bar_diag(p, alpha, y_n, y_n1, gv_mag)
        err = np.abs((y_n1.astype(LD) - y_n.astype(LD)) - LD(alpha) * (lik + gv))
        ratio = float(np.max(err / bar))
        step = float(np.max(np.abs(y_n1 - y_n)) / np.max(np.abs(y_n)))
        print(f"GVDSTEP {label} {case.id} alpha={alpha:g} n={n}: error/bar {ratio:.2e}  (step {step:.2e} of max|y|, K = {K}, "
              f"{gd.gvd_resident(D, T)} arrays resident)")
        if n == 0:      # the GV term is zero by construction at the start
            assert np.all(alpha * np.abs(gv) <= K * EPS * alpha * gv_mag), f"{label}: the GV term at the eq. (58) start"
        assert ratio <= 1.0, f"{label} {case.id} n={n}: error / bar = {ratio:.3g}"


def _single(vc, case, tgv):
    XT = np.asfortranarray(gd.inputs(case)["X"].T)
    return lambda n: vc.fvconvert(tgv, XT, epochs=n, alpha=case.alpha)


# ------------------------------------------------------------------------------------------------ 1. the step check
@pytest.mark.parametrize("case", gd.CASES, ids=lambda c: c.id)
def test_steps(vc, case):
    """the shapes of gv_diag_restatement.SHAPES, every form of the launch rule among them (printed per case)"""
    tgv = _converter(vc, case, case.T)
    assert vc.dim(tgv) == 2 * case.D and vc.ncomponents(tgv) == case.M and len(tgv) == case.T
    if case.ns == gd.N_SHORT:
        assert max(case.ns) + 1 <= 3
    _check_steps(case, _single(vc, case, tgv), "single")


def test_the_cases_cover_every_form_and_both_parities():
    assert {gd.gvd_resident(c.D, c.T) for c in gd.CASES} == {0, 2, 3, 4, 5}
    for ns in (gd.N_FULL, gd.N_SHORT):
        assert {n % 2 for n in ns} | {(n + 1) % 2 for n in ns} == {0, 1}


# ------------------------------------------------------------------------------------------------ 2. a batch
@pytest.mark.parametrize("kind", KINDS)
def test_batch_members(vc, kind):
    """808, 807 and 324 frames in ONE fvconvert_batch call: the batch runs streamed (its longest member), the members alone run
    with two and four arrays resident -- the step check on every member, and every member's bits are its single call's"""
    cases = gd.BATCH_CASES[kind]
    assert len({c.T for c in cases}) == 3 and len({(c.D, c.M, c.alpha, c.cov_scale) for c in cases}) == 1
    assert sorted(gd.gvd_resident(c.D, c.T) for c in cases) == [0, 2, 4] and gd.gvd_resident(cases[0].D, max(c.T for c in cases)) == 0
    tgv = _converter(vc, cases[0], max(c.T for c in cases))
    XTs = [np.asfortranarray(gd.inputs(c)["X"].T) for c in cases]

    @functools.lru_cache(maxsize=None)
    def batch(n):
        return tgv.fvconvert_batch(XTs, epochs=n, alpha=cases[0].alpha)

    for i, c in enumerate(cases):
        seen = set()

        def convert(n, i=i, seen=seen, c=c):   # the first request for n: the shared call; the repeat: the member's single call
            if n in seen:
                return vc.fvconvert(tgv, XTs[i], epochs=n, alpha=c.alpha)
            seen.add(n)
            return batch(n)[i]

        _check_steps(c, convert, f"batch[{i}]")


# ------------------------------------------------------------------------------------------------ 3. bits
@pytest.mark.parametrize("kind", KINDS)
def test_repeats_a_second_stream_and_other_converters_leave_the_bits_alone(vc, kind):
    """D = 12, M = 4, T = 50 and 17 in one batch, 7 epochs; in between: the plain converter under it, a full-mode GV converter
    of another shape, a diagonal GV converter of another shape, and the same handle on other sizes and epoch counts"""
    import torch
    c50, c17 = (next(c for c in gd.CASES if (c.kind, c.D, c.T) == (kind, 12, T)) for T in (50, 17))
    inp = gd.inputs(c50)
    XTs = [np.asfortranarray(inp["X"].T), np.asfortranarray(gd.inputs(c17)["X"].T)]
    tgv = _converter(vc, c50, 50)
    first = tgv.fvconvert_batch(XTs, epochs=7, alpha=c50.alpha)
    fm = np.asfortranarray(np.vstack([np.arange(50.0)[None, :], XTs[0]]))
    dfm = torch.from_numpy(np.ascontiguousarray(fm.T)).cuda().t()
    dev0 = tgv._vc(dfm, epochs=7, alpha=c50.alpha).cpu().numpy()
    assert _same_bits(dev0[1:], first[0])
    full = gr.GV2_CASES[5]                      # D = 13, M = 3, T = 40 in the full mode
    other = next(c for c in gd.CASES if (c.kind, c.D, c.T) == ("dense" if kind == "bdiag" else "bdiag", 33, 65))

    def full_mode():
        i = gr.inputs(full)
        t = vc.TrajectoryGVGMMMap(vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*i["model"])), full.T), i["muv"], np.asfortranarray(i["Sv"]))
        return vc.fvconvert(t, np.asfortranarray(i["X"].T), epochs=3, alpha=full.alpha)

    others = [lambda: vc.fvconvert(tgv.tgmm, XTs[0]), full_mode,
              lambda: _single(vc, other, _converter(vc, other, other.T))(2),
              lambda: tgv.fvconvert_batch(XTs[1:], epochs=4, alpha=c50.alpha),     # (the batch entry leaves len(tgv) alone)
              lambda: tgv.fvconvert_batch(XTs[::-1], epochs=0, alpha=c50.alpha)]
    for f in others:
        f()
        got = tgv.fvconvert_batch(XTs, epochs=7, alpha=c50.alpha)
        assert all(_same_bits(a, b) for a, b in zip(got, first))
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        dev1 = tgv._vc(dfm, epochs=7, alpha=c50.alpha)
    s1.synchronize()
    assert _same_bits(dev1.cpu().numpy(), dev0)
    again = _converter(vc, c50, 50).fvconvert_batch(XTs, epochs=7, alpha=c50.alpha)             # a second handle
    assert all(_same_bits(a, b) for a, b in zip(again, first))


# ------------------------------------------------------------------------------------------------ 4. the reference's own statement
def test_against_the_oracle_and_the_full_mode_detour_on_the_expanded_model(vc):
    """cross-diagonal model, D = 12, L = 50, the reference's defaults alpha = 1e-5 and 100 epochs: oracle/np_oracle.py's GV
    converter on expand_block_diag of the same model, and the full-mode detour on the device, each within 1e-6 of max |y| (the
    tolerance of tests/test_gpu_gv.py for this comparison)"""
    from oracle import np_oracle as npo
    case = next(c for c in gd.CASES if (c.kind, c.D, c.T) == ("bdiag", 12, 50))
    inp = gd.inputs(case)
    w, mu, cov = inp["model"]
    X, muv, Sv = inp["X"], inp["muv"], inp["Sv"]
    y = vc.fvconvert(_converter(vc, case, 50), np.asfortranarray(X.T), epochs=100, alpha=1.0e-5).T
    tj = npo.TrajectoryGMMMap(npo.GMMMap(*tb.expanded_model(w, mu, cov)))
    want = npo.trajgv_fvconvert(tj, X, muv, Sv, epochs=100, alpha=1.0e-5)
    e = float(np.max(np.abs(y - want)) / np.max(np.abs(want)))
    detour = vc.TrajectoryGVGMMMap(vc.TrajectoryGMMMap(vc.GMMMap(w, mu, vc.expand_block_diag(cov)), 50), muv, np.asfortranarray(Sv))
    yd = vc.fvconvert(detour, np.asfortranarray(X.T), epochs=100, alpha=1.0e-5).T
    ed = float(np.max(np.abs(y - yd)) / np.max(np.abs(yd)))
    print(f"GVD against the oracle on the expanded model {e:.2e}, against the full-mode detour {ed:.2e}")
    assert e < 1e-6 and ed < 1e-6
    plain = vc.fvconvert(_traj(vc, "bdiag", inp["model"], 50), np.asfortranarray(X.T)).T
    assert float(np.max(np.abs(y - plain)) / np.max(np.abs(plain))) > 1e-3       # ... about a conversion that GV changes


# ------------------------------------------------------------------------------------------------ 5. the vc surface
@pytest.mark.parametrize("kind", KINDS)
def test_vc_surface_is_the_chunks_converted_one_by_one(vc, kind):
    """D = 12, M = 4, T = 100 in chunks of len(c) = 30 (three whole chunks and a tail of 10), the defaults epochs = 100 and
    alpha = 1e-5: every vc entry equals, bit for bit, fvconvert of the chunks assembled by hand"""
    import torch
    from oracle import np_oracle as npo
    case = next(c for c in gd.CASES if (c.kind, c.D, c.T) == (kind, 12, 50))
    inp = gd.inputs(case)
    D, T, L = 12, 100, 30
    static = gd.utterance(kind, inp["model"], D, case.M, "runs", T)[0][:, :D]
    X = npo.push_delta(static)
    power = np.linspace(-3.0, 2.0, T)
    fm_static = np.asfortranarray(np.vstack([power[None], static.T]))
    fm = np.asfortranarray(np.vstack([power[None], X.T]))
    fresh = lambda: _converter(vc, case, L)                                   # noqa: E731  (vc leaves len(c) at the tail's length)

    def by_hand(Xu, pw, pf=None):
        c = fresh()
        ys = [vc.fvconvert(c, np.asfortranarray(Xu[b:b + L].T)) for b in range(0, Xu.shape[0], L)]
        y = np.asfortranarray(np.hstack(ys))
        if pf is not None:
            y = vc.fvpostf(pf, y)
        return np.asfortranarray(np.vstack([pw[None], y]))

    want = by_hand(X, power)
    assert _same_bits(vc.vc(fresh(), fm), want)
    assert _same_bits(vc.vc(fresh(), fm_static, delta=True), want)
    vs = vc.VarianceScaling(np.var(want[1:], axis=1, ddof=1) * np.linspace(0.5, 2.0, D))
    wantf = by_hand(X, power, vs)
    assert not _same_bits(wantf, want)
    assert _same_bits(vc.vc(fresh(), fm_static, postfilter=vs, delta=True), wantf)
    assert _same_bits(vc.vc(fresh(), fm, postfilter=vs), wantf)
    # a device tensor
    dfm = torch.from_numpy(np.ascontiguousarray(fm_static.T)).cuda().t()
    outd = vc.vc(fresh(), dfm, delta=True)
    assert outd.is_cuda and _same_bits(outd.cpu().numpy(), want)
    outd = vc.vc(fresh(), dfm, postfilter=vs, delta=True)
    assert _same_bits(outd.cpu().numpy(), wantf)
    # vc_batch: three utterances, one of them empty; host matrices and device tensors
    fms = [fm_static, np.zeros((D + 1, 0), order="F"), np.asfortranarray(fm_static[:, :37])]
    w37 = {None: by_hand(npo.push_delta(static[:37]), power[:37]), vs: by_hand(npo.push_delta(static[:37]), power[:37], vs)}
    for pf in (None, vs):
        c = fresh()
        outs = vc.vc_batch(c, fms, postfilter=pf, delta=True)
        assert len(c) == L and outs[1].shape == (D + 1, 0)
        assert _same_bits(outs[0], want if pf is None else wantf) and _same_bits(outs[2], w37[pf])
    douts = vc.vc_batch(fresh(), [dfm, dfm[:, :37]], delta=True)
    assert _same_bits(douts[0].cpu().numpy(), want) and _same_bits(douts[1].cpu().numpy(), w37[None])


# ------------------------------------------------------------------------------------------------ 6. what is refused
def test_refusals(vc):
    import torch
    case = next(c for c in gd.CASES if (c.kind, c.D, c.T) == ("dense", 12, 50))
    inp = gd.inputs(case)
    muv, Sv = inp["muv"], np.asfortranarray(inp["Sv"])
    X = np.asfortranarray(inp["X"].T)
    # over a full-precision converter: at construction
    t = _traj(vc, "dense", inp["model"], 50)
    t.precision = "full"
    with pytest.raises(vc.VCMIError, match="vcmi_trajgv_create"):
        vc.DiagTrajectoryGVGMMMap(t, muv, Sv)
    t.precision = "diag"
    tgv = vc.DiagTrajectoryGVGMMMap(t, muv, Sv)
    before = vc.fvconvert(tgv, X, epochs=5, alpha=case.alpha)
    # the converter switched back to full: every convert entry raises, nothing is written
    t.precision = "full"
    fm = np.asfortranarray(np.vstack([np.ones((1, 50)), X]))
    dfm = torch.from_numpy(np.ascontiguousarray(fm.T)).cuda().t()
    entries = [lambda: vc.fvconvert(tgv, X, epochs=5), lambda: tgv.fvconvert_batch([X, X], epochs=5), lambda: vc.vc(tgv, fm),
               lambda: tgv._vc(fm, vc.VarianceScaling(muv)), lambda: tgv._vc(np.asfortranarray(fm[:13]), delta=True), lambda: vc.vc(tgv, dfm),
               lambda: vc.vc_batch(tgv, [fm, fm]), lambda: vc.vc_batch(tgv, [dfm, dfm])]
    for f in entries:
        with pytest.raises(vc.VCMIError, match="vcmi_trajgv_create"):
            f()
    _lib = __import__("voiceconversion_jl_amd")._lib
    Y = np.full((12, 50), 7.5, order="F")
    rc = _lib.lib.vcmi_trajgv_convert(tgv._h, _lib.dptr(X), 50, 5, case.alpha, _lib.dptr(Y))
    assert rc != 0 and np.all(Y == 7.5)
    assert vc.fvconvert(t, X).shape == (12, 50)                              # (the full-precision converter itself works)
    # ... and after the switch back it converts to the same bits as before
    t.precision = "diag"
    assert _same_bits(vc.fvconvert(tgv, X, epochs=5, alpha=case.alpha), before)
    # one frame has no variance
    with pytest.raises(vc.DimensionMismatch):
        vc.fvconvert(tgv, np.asfortranarray(X[:, :1]), epochs=2)
    with pytest.raises(vc.DimensionMismatch):
        tgv.fvconvert_batch([X, np.asfortranarray(X[:, :1])], epochs=2)
    assert _same_bits(vc.fvconvert(tgv, X, epochs=5, alpha=case.alpha), before)
    # an old-style handle over the same converter still refuses, for both kinds
    for tt in (t, _traj(vc, "bdiag", gd.inputs(next(c for c in gd.CASES if (c.kind, c.D, c.T) == ("bdiag", 12, 50)))["model"], 50)):
        old = vc.TrajectoryGVGMMMap(tt, muv, Sv)
        with pytest.raises(vc.VCMIError, match="diagonal"):
            vc.fvconvert(old, X, epochs=3)
    # the checks of the constructor are TrajectoryGVGMMMap's
    with pytest.raises(AssertionError):
        vc.DiagTrajectoryGVGMMMap(t, -muv, Sv)
    with pytest.raises(vc.PosDefException):
        vc.DiagTrajectoryGVGMMMap(t, muv, np.zeros((12, 12), order="F"))
    with pytest.raises(vc.DimensionMismatch):
        vc.DiagTrajectoryGVGMMMap(t, muv[:-1], Sv)
    assert isinstance(tgv, vc.TrajectoryGVGMMMap) and vc.DiagTrajectoryGVGMMMap.fvconvert_batch is vc.TrajectoryGVGMMMap.fvconvert_batch

