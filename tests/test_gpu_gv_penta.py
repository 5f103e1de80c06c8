"""GPU: BlockDiagTrajectoryGVGMMMap -- the GV ascent over a converter with three windows (csrc/traj_gv_band.hip:
traj_gvp_kernel, behind the pentadiagonal solve), and the same class over two windows.

The step check is tests/test_gpu_gv_diag.py's: for epoch counts n,

    y_n = fvconvert(tgv, X, epochs=n, alpha),  y_{n+1} = the same call with n + 1      (the n call is repeated: same bits)
    | (y_{n+1} - y_n) - alpha (lik + gv)(y_n) |  <=  bar        element by element,

the gradient from tests/gv_penta_restatement.py in long double AT THE DEVICE'S OWN y_n (lik through W and W' as operators, the
form tests/test_gv_penta_restatement_host.py pins to the explicit W; gv from gv_restatement.gv_term, unchanged), and

    bar = K 2^-53 ( |y_n| + |y_{n+1}| + alpha (lik_mag + gv_mag) ),     K = 3 * 3D + T + D + 16,

gv_restatement.step_bar's, fed the five-point lik_magnitude with Emag = |mu^y| + |a| |x - mu^x| for |E| (gv_penta_restatement's
docstring derives the chain length and the magnitude).  Inputs, alpha and the GV covariance scale per case come from the host
(tests/test_gv_penta_restatement_host.py shows both summands visible and every mutant a hundred bars off); odd and even epoch
counts are both among n and n + 1: the parity of the Jacobi buffers decides where the result lands.

Every test here needs BlockDiagTrajectoryGVGMMMap (vcmi_trajgv_create_bdiag) and fails without it.

Measured on an MI355X (figures, not bounds): see the tables of DESIGN 3.5-BDIAG-W3."""
import functools

import numpy as np
import pytest

import gv_diag_restatement as gd
import gv_penta_restatement as gp
import gv_restatement as gr
import traj_diag_restatement as DR
from conftest import relerr
from gv_restatement import EPS, LD
from oracle import np_oracle as npo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def _traj(vc, model, L):
    return vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(*model), L, windows=3)


def _converter(vc, case, L):
    inp = gp.inputs(case)
    return vc.BlockDiagTrajectoryGVGMMMap(_traj(vc, inp["model"], L), inp["muv"], np.asfortranarray(inp["Sv"]))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_steps(case, convert, label):
    """convert(n) -> y_n (D,T) of the case's utterance; the step check at every n of case.ns"""
    p = gp.inputs(case)["pieces"]
    D, T, alpha = case.D, case.T, case.alpha
    ys = {n: convert(n) for n in sorted(set(case.ns) | {n + 1 for n in case.ns})}
    K = gp.chain_length(p)
    assert K == 9 * D + T + D + 16
    for n in case.ns:
        assert _same_bits(convert(n), ys[n]), f"{label}: epochs={n} twice gives different bits"
        y_n, y_n1 = np.asarray(ys[n]).T, np.asarray(ys[n + 1]).T
        assert y_n.shape == (T, D) and np.all(np.isfinite(y_n)) and np.all(np.isfinite(y_n1))
        lik, gv, _, gv_mag = gp.gradient_terms(p, y_n, mags=False)
        bar = gp.step_bar(p, alpha, y_n, y_n1, gv_mag)
        err = np.abs((y_n1.astype(LD) - y_n.astype(LD)) - LD(alpha) * (lik + gv))
        ratio = float(np.max(err / bar))
        step = float(np.max(np.abs(y_n1 - y_n)) / np.max(np.abs(y_n)))
        print(f"GVPSTEP {label} {case.id} alpha={alpha:g} n={n}: error/bar {ratio:.2e}  (step {step:.2e} of max|y|, K = {K}, "
              f"{gp.gvp_resident(D, T)} arrays resident)")
        if n == 0:      # the GV term is zero by construction at the start
            assert np.all(alpha * np.abs(gv) <= K * EPS * alpha * gv_mag), f"{label}: the GV term at the eq. (58) start"
        assert ratio <= 1.0, f"{label} {case.id} n={n}: error / bar = {ratio:.3g}"


def _single(vc, case, tgv):
    XT = np.asfortranarray(gp.inputs(case)["X"].T)
    return lambda n: vc.fvconvert(tgv, XT, epochs=n, alpha=case.alpha)


# ------------------------------------------------------------------------------------------------ 1. the step check
@pytest.mark.parametrize("case", gp.CASES, ids=lambda c: c.id)
def test_steps(vc, case):
    """the shapes of gv_penta_restatement.SHAPES, every form of the launch rule among them (printed per case)"""
    tgv = _converter(vc, case, case.T)
    assert vc.dim(tgv) == 3 * case.D and vc.ncomponents(tgv) == case.M and len(tgv) == case.T and tgv.tgmm.windows == 3
    if case.ns == gp.N_SHORT:
        assert max(case.ns) + 1 <= 3
    _check_steps(case, _single(vc, case, tgv), "single")


# ------------------------------------------------------------------------------------------------ 2. a batch
def test_batch_members(vc):
    """808, 807 and 270 frames in ONE fvconvert_batch call: the batch runs streamed (its longest member), the members alone run
    with two and five arrays resident -- the step check on every member, and every member's bits are its single call's"""
    cases = gp.BATCH_CASES
    assert len({c.T for c in cases}) == 3 and len({(c.D, c.M, c.alpha, c.cov_scale) for c in cases}) == 1
    assert sorted(gp.gvp_resident(c.D, c.T) for c in cases) == [0, 2, 5] and gp.gvp_resident(cases[0].D, max(c.T for c in cases)) == 0
    tgv = _converter(vc, cases[0], max(c.T for c in cases))
    XTs = [np.asfortranarray(gp.inputs(c)["X"].T) for c in cases]

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
def test_repeats_a_second_stream_and_other_converters_leave_the_bits_alone(vc):
    """D = 12, M = 4, T = 50 and 17 in one batch, 7 epochs; in between: the plain converter under it, a two-window GV converter, a
    three-window GV converter of another shape, and the same handle on other sizes and epoch counts"""
    import torch
    c50, c17 = (next(c for c in gp.CASES if (c.D, c.T) == (12, T)) for T in (50, 17))
    inp = gp.inputs(c50)
    XTs = [np.asfortranarray(inp["X"].T), np.asfortranarray(gp.inputs(c17)["X"].T)]
    tgv = _converter(vc, c50, 50)
    first = tgv.fvconvert_batch(XTs, epochs=7, alpha=c50.alpha)
    fm = np.asfortranarray(np.vstack([np.arange(50.0)[None, :], XTs[0]]))
    dfm = torch.from_numpy(np.ascontiguousarray(fm.T)).cuda().t()
    dev0 = tgv._vc(dfm, epochs=7, alpha=c50.alpha).cpu().numpy()
    assert _same_bits(dev0[1:], first[0])
    two = next(c for c in gd.CASES if (c.kind, c.D, c.T) == ("bdiag", 33, 65))
    other = next(c for c in gp.CASES if (c.D, c.T) == (33, 65))

    def two_windows():
        i = gd.inputs(two)
        t = vc.BlockDiagTrajectoryGVGMMMap(vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(*i["model"]), two.T), i["muv"],
                                           np.asfortranarray(i["Sv"]))
        return vc.fvconvert(t, np.asfortranarray(i["X"].T), epochs=3, alpha=two.alpha)

    others = [lambda: vc.fvconvert(tgv.tgmm, XTs[0]), two_windows,
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


# ------------------------------------------------------------------------------------------------ 4. epochs = 0 and the whole ascent
@pytest.mark.parametrize("D,T", [(12, 2), (12, 50), (33, 65), (40, 300), (42, 33), (12, 808)])
def test_epochs_0_is_the_rescaled_plain_trajectory(vc, D, T):
    """eq. (58) applied to what the pentadiagonal solve left: variance_scaling of the plain three-window result, within the
    solver's own bound 64 cond rho 2^-53 (tests/traj_penta_restatement.py) -- the rescale maps a relative difference of the plain
    trajectory into the same relative difference (mean and scale are smooth in y), with the factor 2 for its two uses of y"""
    case = next(c for c in gp.CASES if (c.D, c.T) == (D, T))
    inp = gp.inputs(case)
    tgv = _converter(vc, case, T)
    X = np.asfortranarray(inp["X"].T)
    y0 = vc.fvconvert(tgv, X, epochs=0).T
    plain = vc.fvconvert(tgv.tgmm, X).T
    bound = DR.tolerance(inp["cond"]) * inp["rho"]
    e_dev, e_ref = relerr(y0, npo.variance_scaling(plain, inp["muv"])), relerr(y0, inp["y0"])
    print(f"GVP epochs=0 D={D} T={T}: against variance_scaling of the device's plain result {e_dev:.2e}, of the restatement's "
          f"{e_ref:.2e}, bound {bound:.2e}")
    assert e_dev < bound and e_ref < 2 * bound
    assert np.allclose(y0.var(axis=0, ddof=1), inp["muv"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("D,T", [(12, 50), (33, 65), (40, 300)])
def test_whole_ascent_against_the_restatement_iterated_in_fp64(vc, D, T):
    """20 epochs at the case's step-visible alpha against gv_penta_restatement.ascent(fp64=True) from the restatement's own plain
    trajectory; the bar on the increments y_20 - y_0 is gv_penta_restatement.increment_bar (gv_restatement.increment_bar's
    form with the pentadiagonal system's condition number and rho)"""
    case = next(c for c in gp.CASES if (c.D, c.T) == (D, T))
    inp = gp.inputs(case)
    epochs = 20
    want, _ = gp.ascent(inp["pieces"], inp["y0"], epochs, case.alpha, fp64=True)
    want = want.astype(np.float64)
    tgv = _converter(vc, case, T)
    X = np.asfortranarray(inp["X"].T)
    y, y0 = vc.fvconvert(tgv, X, epochs=epochs, alpha=case.alpha).T, vc.fvconvert(tgv, X, epochs=0).T
    inc_ref, inc = want - inp["y0"], y - y0
    bar = gp.increment_bar(inp["cond"], inp["rho"], want, inp["y0"], inp["y_ml"], inc_ref, inp["muv"])
    err = float(np.max(np.abs(inc - inc_ref)) / np.max(np.abs(inc_ref)))
    print(f"GVP ascent D={D} T={T}: increment error {err:.2e}, bar {bar:.2e} (cond {inp['cond']:.1f}, rho {inp['rho']:.2f}); "
          f"max|inc|/max|y| {float(np.max(np.abs(inc_ref)) / np.max(np.abs(want))):.2e}")
    assert float(np.max(np.abs(inc_ref)) / np.max(np.abs(want))) > 1e-4        # ... about an ascent that moves
    assert err <= bar


# ------------------------------------------------------------------------------------------------ 5. two windows
def test_two_windows_is_diag_trajectory_gv_bit_for_bit(vc):
    """over a two-window BlockDiagTrajectoryGMMMap the new class is DiagTrajectoryGVGMMMap: fvconvert, a batch, vc with a
    post-filter"""
    case = next(c for c in gd.CASES if (c.kind, c.D, c.T) == ("bdiag", 12, 50))
    c17 = next(c for c in gd.CASES if (c.kind, c.D, c.T) == ("bdiag", 12, 17))
    inp = gd.inputs(case)
    muv, Sv = inp["muv"], np.asfortranarray(inp["Sv"])
    mk = lambda cls, L: cls(vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(*inp["model"]), L), muv, Sv)      # noqa: E731
    XTs = [np.asfortranarray(inp["X"].T), np.asfortranarray(gd.inputs(c17)["X"].T)]
    a, b = mk(vc.BlockDiagTrajectoryGVGMMMap, 50), mk(vc.DiagTrajectoryGVGMMMap, 50)
    assert isinstance(a, vc.DiagTrajectoryGVGMMMap) and a.tgmm.windows == 2
    for n in (0, 1, 8):
        assert _same_bits(vc.fvconvert(a, XTs[0], epochs=n, alpha=case.alpha), vc.fvconvert(b, XTs[0], epochs=n, alpha=case.alpha))
    assert all(_same_bits(x, y) for x, y in zip(a.fvconvert_batch(XTs, epochs=5, alpha=case.alpha),
                                                b.fvconvert_batch(XTs, epochs=5, alpha=case.alpha)))
    fm = np.asfortranarray(np.vstack([np.linspace(-3.0, 2.0, 50)[None], XTs[0]]))
    vs = vc.VarianceScaling(muv * np.linspace(0.5, 2.0, 12))
    assert _same_bits(vc.vc(mk(vc.BlockDiagTrajectoryGVGMMMap, 30), fm, postfilter=vs), vc.vc(mk(vc.DiagTrajectoryGVGMMMap, 30), fm, postfilter=vs))
    st = np.asfortranarray(fm[:13])
    assert _same_bits(vc.vc(mk(vc.BlockDiagTrajectoryGVGMMMap, 30), st, postfilter=vs, delta=True),
                      vc.vc(mk(vc.DiagTrajectoryGVGMMMap, 30), st, postfilter=vs, delta=True))


# ------------------------------------------------------------------------------------------------ 6. the vc surface
def test_vc_surface_is_the_chunks_converted_one_by_one(vc):
    """D = 12, M = 4, T = 100 in chunks of len(c) = 30 (three whole chunks and a tail of 10), the defaults epochs = 100 and
    alpha = 1e-5: the host (3D+1,T) matrix and the device tensor, with and without VarianceScaling, equal, bit for bit,
    fvconvert of the chunks assembled by hand"""
    import torch
    case = next(c for c in gp.CASES if (c.D, c.T) == (12, 50))
    inp = gp.inputs(case)
    D, T, L = 12, 100, 30
    X = gp.utterance(inp["model"], D, case.M, "runs", T)[0]
    power = np.linspace(-3.0, 2.0, T)
    fm = np.asfortranarray(np.vstack([power[None], X.T]))
    fresh = lambda: _converter(vc, case, L)                                   # noqa: E731  (vc leaves len(c) at the tail's length)

    def by_hand(pf=None):
        c = fresh()
        ys = [vc.fvconvert(c, np.asfortranarray(X[b:b + L].T)) for b in range(0, T, L)]
        y = np.asfortranarray(np.hstack(ys))
        if pf is not None:
            y = vc.fvpostf(pf, y)
        return np.asfortranarray(np.vstack([power[None], y]))

    want = by_hand()
    assert want.shape == (D + 1, T) and _same_bits(vc.vc(fresh(), fm), want)
    plain = vc.vc(_traj(vc, inp["model"], L), fm)
    assert _same_bits(plain[0], want[0]) and not _same_bits(plain, want)      # (GV changes the conversion)
    vs = vc.VarianceScaling(np.var(want[1:], axis=1, ddof=1) * np.linspace(0.5, 2.0, D))
    wantf = by_hand(vs)
    assert not _same_bits(wantf, want)
    c = fresh()
    assert _same_bits(vc.vc(c, fm, postfilter=vs), wantf) and len(c) == 10
    # non-default epochs / alpha take the one-call entry on the host matrix too
    c = fresh()
    ys = [vc.fvconvert(c, np.asfortranarray(X[b:b + L].T), epochs=3, alpha=case.alpha) for b in range(0, T, L)]
    assert _same_bits(fresh()._vc(fm, epochs=3, alpha=case.alpha)[1:], np.hstack(ys))
    # a device tensor
    dfm = torch.from_numpy(np.ascontiguousarray(fm.T)).cuda().t()
    outd = vc.vc(fresh(), dfm)
    assert outd.is_cuda and _same_bits(outd.cpu().numpy(), want)
    outd = vc.vc(fresh(), dfm, postfilter=vs)
    assert _same_bits(outd.cpu().numpy(), wantf)


# ------------------------------------------------------------------------------------------------ 7. what is refused
def test_refusals_leave_a_working_handle(vc):
    import torch
    case = next(c for c in gp.CASES if (c.D, c.T) == (12, 50))
    inp = gp.inputs(case)
    D = 12
    muv, Sv = inp["muv"], np.asfortranarray(inp["Sv"])
    X = np.asfortranarray(inp["X"].T)
    tgv = _converter(vc, case, 50)
    before = vc.fvconvert(tgv, X, epochs=5, alpha=case.alpha)

    def still_converts():
        assert len(tgv) == 50 and _same_bits(vc.fvconvert(tgv, X, epochs=5, alpha=case.alpha), before)

    three = "three windows"
    static = np.asfortranarray(np.vstack([np.ones((1, 50)), X[:D]]))
    fm = np.asfortranarray(np.vstack([np.ones((1, 50)), X]))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()    # noqa: E731
    # static input, host and device
    for f in (lambda: vc.vc(tgv, static, delta=True), lambda: vc.vc(tgv, static, postfilter=vc.VarianceScaling(muv), delta=True),
              lambda: vc.vc(tgv, dev(static), delta=True)):
        with pytest.raises(vc.VCMIError, match=three):
            f()
    still_converts()
    # the batch family
    for fms in ([fm, fm], [static, static], [dev(fm), dev(fm)]):
        with pytest.raises(vc.VCMIError, match=three):
            vc.vc_batch(tgv, fms, delta=fms[0].shape[0] == D + 1)
    still_converts()
    # a converter that is not cross-diagonal: TypeError from the class, VCMI_ERR_ARG naming the two other constructors from the entry
    di = gd.inputs(next(c for c in gd.CASES if (c.kind, c.D, c.T) == ("dense", 12, 50)))
    from conftest import julia_model
    dense = vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*di["model"])), 50, precision="diag")
    with pytest.raises(TypeError, match="BlockDiagTrajectoryGMMMap"):
        vc.BlockDiagTrajectoryGVGMMMap(dense, di["muv"], np.asfortranarray(di["Sv"]))
    import ctypes as C
    _lib = __import__("voiceconversion_jl_amd")._lib
    h = C.c_void_p()
    rc = _lib.lib.vcmi_trajgv_create_bdiag(dense._h, _lib.dptr(di["muv"]), _lib.dptr(np.asfortranarray(di["Sv"])), C.byref(h))
    assert rc != 0 and not h
    with pytest.raises(vc.VCMIError, match="vcmi_trajgv_create_diag") as ei:
        _lib.check(rc)
    assert "vcmi_trajgv_create or" in str(ei.value)
    assert vc.fvconvert(vc.DiagTrajectoryGVGMMMap(dense, di["muv"], np.asfortranarray(di["Sv"])), np.asfortranarray(di["X"].T), epochs=2).shape == (12, 50)
    still_converts()
    # one frame has no variance
    with pytest.raises(vc.DimensionMismatch):
        vc.fvconvert(tgv, np.asfortranarray(X[:, :1]), epochs=2)
    with pytest.raises(vc.DimensionMismatch):
        tgv.fvconvert_batch([X, np.asfortranarray(X[:, :1])], epochs=2)
    with pytest.raises(vc.VCMIError, match="negative epoch"):
        vc.fvconvert(tgv, X, epochs=-1)
    Y = np.full((12, 50), 7.5, order="F")
    rc = _lib.lib.vcmi_trajgv_convert(tgv._h, _lib.dptr(np.asfortranarray(X[:, :1])), 1, 5, case.alpha, _lib.dptr(Y))
    assert rc != 0 and np.all(Y == 7.5)
    still_converts()
    # an empty utterance rides in a batch
    ys = tgv.fvconvert_batch([X, np.zeros((3 * D, 0), order="F")], epochs=5, alpha=case.alpha)
    assert ys[1].shape == (D, 0) and _same_bits(ys[0], before)
    # the old constructors over the three-window converter still refuse
    with pytest.raises(vc.VCMIError, match=three):
        vc.DiagTrajectoryGVGMMMap(tgv.tgmm, muv, Sv)
    old = vc.TrajectoryGVGMMMap(tgv.tgmm, muv, Sv)
    with pytest.raises(vc.VCMIError, match="diagonal"):
        vc.fvconvert(old, X, epochs=3)
    still_converts()
    # the checks of the constructor are TrajectoryGVGMMMap's
    with pytest.raises(AssertionError):
        vc.BlockDiagTrajectoryGVGMMMap(tgv.tgmm, -muv, Sv)
    with pytest.raises(vc.PosDefException):
        vc.BlockDiagTrajectoryGVGMMMap(tgv.tgmm, muv, np.zeros((12, 12), order="F"))
    with pytest.raises(vc.DimensionMismatch):
        vc.BlockDiagTrajectoryGVGMMMap(tgv.tgmm, muv[:-1], Sv)
    Sv0 = np.zeros((12, 12), order="F")
    assert _lib.lib.vcmi_trajgv_create_bdiag(tgv.tgmm._h, _lib.dptr(-muv), _lib.dptr(Sv), C.byref(h)) != 0 and not h
    assert _lib.lib.vcmi_trajgv_create_bdiag(tgv.tgmm._h, _lib.dptr(muv), _lib.dptr(Sv0), C.byref(h)) != 0 and not h
    still_converts()
