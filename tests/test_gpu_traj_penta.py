"""GPU: BlockDiagTrajectoryGMMMap(g, T, windows=3) -- trajectory conversion with static + delta + delta-delta features straight
from a cross-diagonal model (vcmi_traj_create_bdiag_windows: the fused arg-max + g_t pass of csrc/gmmmap_bdiag.hip over 3D rows
and the pentadiagonal solver of csrc/traj_penta.hip) -- against the numpy restatement tests/traj_penta_restatement.py.

Tolerance: relerr < 64 cond rho 2^-53, cond the largest condition number of the pentadiagonal systems of the input and rho the
cancellation the centred g can carry into the right-hand side, both as the restatement reports them; derived in its docstring.
tests/test_traj_penta_host.py asserts for every input used here that every q > 0 and that no frame's arg-max is within rounding
of a tie, so both sides take the same mixture sequence."""
import ctypes as C
import functools

import numpy as np
import pytest

import traj_bdiag_restatement as R2
import traj_diag_restatement as DR
import traj_penta_restatement as R
from conftest import relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


@functools.lru_cache(maxsize=None)
def _case(D, M, Ts, swap=False):
    """model, utterances (T,3D), their restated trajectories (Y, cond, rho) and the restatement: made once, never written to"""
    model, Xs = R.make_case(D, M, list(Ts), swap)
    bt = R.PentaTrajectory(*model, swap)
    return model, Xs, [bt.banded(X) for X in Xs], bt


def _conv(vc, model, T, swap=False):
    return vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(*model, swap=swap), T, windows=3)


def _check(y, ref, cond, rho, what="", factor=1.0):
    err = relerr(y, ref) if ref.size else 0.0
    bound = factor * DR.tolerance(cond) * rho
    print(f"{what}: relerr {err:.3e}  cond {cond:.3f}  rho {rho:.3f}  bound {bound:.3e}")
    assert y.shape == ref.shape
    assert err < bound, (what, err, bound)


# ------------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("D,M,Ts", [(D, M, tuple(Ts)) for D, M, Ts in R.SHAPES])
def test_vs_restatement_batch(vc, D, M, Ts):
    """D = 40, M = 8: 3D = 120 features, five 64-frame tiles with a partial last one; T = 1..5: the stencil loses one and two
    neighbours on each side; D = 7: 3D = 21 is padded in the tables; D = 42: the limit 3D = 126 <= 128, T = 64 and 65 fill a tile
    and step one frame past it, T = 1, 2, 3 the shortest chains at the limit; M = 256 at 3D = 12: the pass's 32-frame tiles, 16
    distinct mixtures in the utterance (per-lane gathers in the solver); D = 40, M = 64: the benchmark's model, 19 distinct
    mixtures.  T = 50, 130, 300: several rings of six solver steps and a partial last one.  An empty utterance rides in every
    batch."""
    model, Xs, refs, _ = _case(D, M, Ts)
    t = _conv(vc, model, max(Ts))
    assert t.windows == 3 and t.precision == "diag" and vc.dim(t) == 3 * D and vc.ncomponents(t) == M and len(t) == max(Ts)
    batch = [X.T for X in Xs[:1]] + [np.zeros((3 * D, 0), order="F")] + [X.T for X in Xs[1:]]
    Ys = t.fvconvert_batch(batch)
    assert Ys[1].shape == (D, 0)
    Ys = Ys[:1] + Ys[2:]
    for X, y, (ref, cond, rho) in zip(Xs, Ys, refs):
        _check(y, ref.T, cond, rho, f"D={D} M={M} T={X.shape[0]}")
    # batch == single, bit for bit
    for X, y in zip(Xs, Ys):
        assert np.array_equal(vc.fvconvert(t, X.T), y)


def test_fvconvert_takes_device_tensors(vc):
    """D = 12, M = 4, T = 1..50 and an empty utterance as device tensors, one of them a view with a leading dimension above 3D:
    device tensors come back, bit for bit the host results; a two-window converter takes them too; len(t) is left alone"""
    import torch
    D, M, Ts = 12, 4, (1, 2, 3, 4, 5, 50)
    model, Xs, refs, _ = _case(D, M, Ts)
    t = _conv(vc, model, 50)
    host = t.fvconvert_batch([X.T for X in Xs])
    dXs = [torch.from_numpy(X.copy()).cuda().t() for X in Xs]
    wide = torch.zeros((50, 3 * D + 5), dtype=torch.float64).cuda()
    wide[:, :3 * D] = dXs[-1].t()
    dXs[-1] = wide[:, :3 * D].t()
    dXs.insert(2, torch.zeros((0, 3 * D), dtype=torch.float64).cuda().t())
    got = t.fvconvert_batch(dXs)
    assert got[2].shape == (D, 0) and all(y.is_cuda for y in got) and len(t) == 50
    got = got[:2] + got[3:]
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, host))
    one = vc.fvconvert(t, dXs[0])
    assert one.is_cuda and np.array_equal(one.cpu().numpy(), host[0]) and len(t) == 50
    _check(got[-1].cpu().numpy(), refs[-1][0].T, refs[-1][1], refs[-1][2], "device tensors")
    with pytest.raises(vc.DimensionMismatch):
        t.fvconvert_batch([dXs[0][:2 * D]])
    with pytest.raises(TypeError, match="device tensors and host"):
        t.fvconvert_batch([dXs[0], Xs[1].T])
    two_model, two_Xs = R2.make_case(D, M, list(Ts))
    t2 = vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(*two_model), 50)
    host2 = t2.fvconvert_batch([X.T for X in two_Xs])
    got2 = t2.fvconvert_batch([torch.from_numpy(X.copy()).cuda().t() for X in two_Xs])
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got2, host2))


# ------------------------------------------------------------------------------------------------ 2. the first maximum
def test_first_maximum_rule_and_a_mixture_without_weight(vc):
    """D = 3, M = 3, T = 10 over three windows: mixtures 1 and 2 have bit-identical weights and source sides and different target
    sides: the result is the restatement's with mhat = the lower index.  Mixture 3 sits on the frames' own mean and has weight 0."""
    model, X = R.tie_case()
    bt = R.PentaTrajectory(*model)
    g = vc.BlockDiagGMMMap(*model)
    assert np.all(vc.predict(g.px, X.T) == 1)
    y = vc.fvconvert(vc.BlockDiagTrajectoryGMMMap(g, 10, windows=3), X.T)
    ref, cond, rho = bt.banded(X, mhat=np.ones(10, dtype=np.int64))
    _check(y, ref.T, cond, rho, "tie -> mixture 1")
    other = bt.banded(X, mhat=np.full(10, 2))[0]
    assert relerr(y, other.T) > 1e-3


# ------------------------------------------------------------------------------------------------ 3. swap
def test_swap(vc):
    """the (12, 4) shape with the halves of the model exchanged: source = rows 3D .. 6D-1"""
    D, M, Ts = 12, 4, (1, 2, 3, 4, 5, 50)
    model, Xs, refs, _ = _case(D, M, Ts, True)
    t = _conv(vc, model, 50, swap=True)
    for X, y, (ref, cond, rho) in zip(Xs, t.fvconvert_batch([X.T for X in Xs]), refs):
        _check(y, ref.T, cond, rho, f"swap T={X.shape[0]}")
    unswapped = vc.fvconvert(_conv(vc, model, 50), Xs[-1].T)
    assert relerr(unswapped, refs[-1][0].T) > 1e-3


# ------------------------------------------------------------------------------------------------ 4. the vc surface
def test_vc_surface_against_the_restatement_chunk_by_chunk(vc):
    """D = 12, M = 4, T = 100 in chunks of len(c) = 30: three whole chunks and a tail of 10; fm is (3D+1, T)"""
    import torch
    from oracle import np_oracle as npo
    D, M, (T,) = R.VC_CASE
    L = 30
    model, Xs, _, bt = _case(D, M, (T,))
    power = np.linspace(-3.0, 2.0, T)
    full = np.concatenate([power[:, None], Xs[0]], axis=1)                    # (T, 3D+1)
    want, cond, rho = bt.vc(full, L)
    fresh = lambda: _conv(vc, model, L)                                       # noqa: E731  (vc leaves len(c) at the tail's length)
    c = fresh()
    out = vc.vc(c, np.asfortranarray(full.T))
    assert out.shape == (D + 1, T) and np.array_equal(out[0], full[:, 0]) and len(c) == 10
    _check(out[1:], want[:, 1:].T, cond, rho, "vc(t, fm)")
    # a VarianceScaling post-filter over the whole converted utterance
    s2 = np.var(want[:, 1:], axis=0, ddof=1) * np.linspace(0.5, 2.0, D)
    vs = vc.VarianceScaling(s2)
    wantf = npo.variance_scaling(want[:, 1:], s2)
    c = fresh()
    outf = vc.vc(c, np.asfortranarray(full.T), postfilter=vs)
    assert np.array_equal(outf[0], full[:, 0]) and len(c) == 10
    _check(outf[1:], wantf.T, cond, rho, "vc with VarianceScaling")
    # a device tensor, with and without the filter: the host calls bit for bit
    dfm = torch.from_numpy(full.copy()).cuda().t()
    c = fresh()
    outd = vc.vc(c, dfm)
    assert outd.is_cuda and outd.shape == (D + 1, T) and len(c) == 10
    outd = outd.cpu().numpy()
    assert np.array_equal(outd[0], full[:, 0])
    _check(outd[1:], want[:, 1:].T, cond, rho, "vc(t, device fm)")
    assert np.array_equal(outd, out)
    outdf = vc.vc(fresh(), dfm, postfilter=vs).cpu().numpy()
    assert np.array_equal(outdf[0], full[:, 0])
    _check(outdf[1:], wantf.T, cond, rho, "vc(t, device fm) with VarianceScaling")
    assert np.array_equal(outdf, outf)
    # fm with the rows of two windows is not this converter's input
    with pytest.raises(vc.DimensionMismatch):
        vc.vc(fresh(), np.asfortranarray(full[:, :2 * D + 1].T))


# ------------------------------------------------------------------------------------------------ 5. push_delta(order=2)
@pytest.mark.parametrize("T", [1, 2, 3, 50])
def test_push_delta_order_2_on_the_device(vc, T):
    """the device kernel equals the host routine bit for bit, also from a matrix with a leading dimension above D"""
    import torch
    D, ld = 5, 9
    src = np.random.default_rng(70 + T).standard_normal((T, D))
    want = vc.push_delta(np.asfortranarray(src.T), order=2)
    assert np.array_equal(want, R.push_delta2(src).T)
    got = vc.push_delta(torch.from_numpy(src.copy()).cuda().t(), order=2)
    assert got.is_cuda and got.shape == (3 * D, T) and np.array_equal(got.cpu().numpy(), want)
    buf = torch.full((T, ld), np.nan, dtype=torch.float64).cuda()
    buf[:, :D] = torch.from_numpy(src).cuda()
    view = buf[:, :D].t()
    assert T == 1 or view.stride(1) == ld
    got = vc.push_delta(view, order=2)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(got[:2 * D].cpu().numpy(), vc.push_delta(view).cpu().numpy())


# ------------------------------------------------------------------------------------------------ 6. bits
def test_repeats_a_second_stream_and_other_converters_leave_the_bits_alone(vc):
    """D = 12, M = 4, T = 1..50; the other converters in between: a two-window converter, a three-window converter of another
    shape (D = 7), and the frame-by-frame entry of the same BlockDiagGMMMap"""
    import torch
    D, M, Ts = 12, 4, (1, 2, 3, 4, 5, 50)
    model, Xs, _, _ = _case(D, M, Ts)
    batch = [X.T for X in Xs]
    t = _conv(vc, model, 50)
    first = t.fvconvert_batch(batch)
    fm = np.asfortranarray(np.vstack([np.arange(50.0)[None, :], Xs[-1].T]))
    dfm = torch.from_numpy(np.ascontiguousarray(fm.T)).cuda().t()
    dev0 = vc.vc(t, dfm).cpu().numpy()
    assert np.array_equal(dev0[1:], first[-1])
    two_model, two_Xs = R2.make_case(D, M, list(Ts))
    other_model, other_Xs, _, _ = _case(7, 2, (30, 2))
    others = [lambda: vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(*two_model), 50).fvconvert_batch([X.T for X in two_Xs]),
              lambda: _conv(vc, other_model, 30).fvconvert_batch([X.T for X in other_Xs]),
              lambda: vc.fvconvert(t.gmmmap, np.asfortranarray(Xs[-1].T)),
              lambda: t.fvconvert_batch(batch[2:4])]               # (another size: through the batch entry, which leaves len(t))
    for other in others:
        other()
        got = t.fvconvert_batch(batch)
        assert all(np.array_equal(a, b) for a, b in zip(got, first))
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        dev1 = vc.vc(t, dfm)
    s1.synchronize()
    assert np.array_equal(dev1.cpu().numpy(), dev0)
    assert all(np.array_equal(a, b) for a, b in zip(_conv(vc, model, 50).fvconvert_batch(batch), first))     # a second handle


# ------------------------------------------------------------------------------------------------ 7. what is refused
def test_refusals_leave_a_working_handle(vc):
    import torch
    from voiceconversion_jl_amd import _lib
    D, M, Ts = 12, 4, (1, 2, 3, 4, 5, 50)
    model, Xs, refs, _ = _case(D, M, Ts)
    X = np.asfortranarray(Xs[-1].T)
    Y = np.asfortranarray(refs[-1][0].T)
    t = _conv(vc, model, 50)

    def still_converts():
        assert t.windows == 3 and t.precision == "diag" and t.em_iters == 0 and len(t) == 50
        _check(vc.fvconvert(t, X), refs[-1][0].T, refs[-1][1], refs[-1][2], "after a refusal")

    three = "three windows"
    static = np.asfortranarray(np.vstack([np.ones((1, 50)), X[:D]]))         # (D+1, T)
    fm = np.asfortranarray(np.vstack([np.ones((1, 50)), X]))                 # (3D+1, T)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()    # noqa: E731
    # static input, host and device
    with pytest.raises(vc.VCMIError, match=three):
        vc.vc(t, static, delta=True)
    with pytest.raises(vc.VCMIError, match=three):
        vc.vc(t, static, postfilter=vc.VarianceScaling(np.ones(D)), delta=True)
    with pytest.raises(vc.VCMIError, match=three):
        vc.vc(t, dev(static), delta=True)
    still_converts()
    # the batch family
    for fms in ([fm, fm], [static, static], [dev(fm), dev(fm)]):
        with pytest.raises(vc.VCMIError, match=three):
            vc.vc_batch(t, fms, delta=fms[0].shape[0] == D + 1)
    still_converts()
    # EM re-estimation and L(y): the cross-diagonal entries themselves
    with pytest.raises(vc.VCMIError, match=three):
        _lib.check(_lib.lib.vcmi_traj_set_em_bdiag(t._h, 1))
    _lib.check(_lib.lib.vcmi_traj_set_em_bdiag(t._h, 0))                     # (switching it off is no request for EM)
    with pytest.raises(vc.VCMIError, match="diagonal"):                      # ... and the dense model's keep refusing as before
        t.em_iters = 1
    L = C.c_double(0.0)
    with pytest.raises(vc.VCMIError, match=three):
        _lib.check(_lib.lib.vcmi_traj_cond_loglik_bdiag(t._h, _lib.dptr(X), _lib.dptr(Y), 50, C.byref(L)))
    dX, dY, dL = dev(X), dev(Y), torch.zeros(1, dtype=torch.float64).cuda()
    with pytest.raises(vc.VCMIError, match=three):
        _lib.check(_lib.lib.vcmi_traj_cond_loglik_bdiag_dev(t._h, dX.data_ptr(), dY.data_ptr(), 50, dL.data_ptr(), None))
    with pytest.raises(vc.VCMIError, match="cross-diagonal"):
        t.cond_loglik(X, Y)
    still_converts()
    # the GV ascent over diagonal precisions: refused when the handle is made
    muv = np.var(refs[-1][0], axis=0, ddof=1) * 1.2
    with pytest.raises(vc.VCMIError, match=three):
        vc.DiagTrajectoryGVGMMMap(t, muv, np.diag(muv ** 2 * 0.1))
    still_converts()
    with pytest.raises(vc.VCMIError, match="cross-diagonal"):
        t.precision = "full"
    # X with the rows of two windows
    with pytest.raises(vc.DimensionMismatch):
        vc.fvconvert(t, np.zeros((2 * D, 5), order="F"))
    still_converts()


def test_constructor_rules_and_two_windows_through_the_new_entry(vc):
    from em_bdiag_restatement import bdiag_model
    from voiceconversion_jl_amd import _lib
    # windows = 2 through vcmi_traj_create_bdiag_windows is BlockDiagTrajectoryGMMMap(g, T), bit for bit, on the (12, 4) shape
    D, M, Ts = 12, 4, (1, 2, 3, 4, 5, 50)
    model, Xs = R2.make_case(D, M, list(Ts))
    g = vc.BlockDiagGMMMap(*model)
    old = vc.BlockDiagTrajectoryGMMMap(g, 50)
    assert old.windows == 2 and vc.BlockDiagTrajectoryGMMMap(g, 50, windows=2).windows == 2
    new = object.__new__(vc.BlockDiagTrajectoryGMMMap)
    new.gmmmap = g
    h = C.c_void_p()
    _lib.check(_lib.lib.vcmi_traj_create_bdiag_windows(g._h, 50, 2, C.byref(h)))
    new._h = h
    assert new.windows == 2 and vc.dim(new) == 2 * D and len(new) == 50
    batch = [X.T for X in Xs]
    assert all(np.array_equal(a, b) for a, b in zip(new.fvconvert_batch(batch), old.fvconvert_batch(batch)))
    bt = R2.BdiagTrajectory(*model)
    ref, cond, rho = bt.tridiag(Xs[-1])
    _check(vc.fvconvert(new, Xs[-1].T), ref.T, cond, rho, "windows=2 through the new entry")
    # dim(g) = 24 is even and a multiple of 3: the same model is a two-window converter of D = 12 and a three-window one of D = 8
    t3 = vc.BlockDiagTrajectoryGMMMap(g, 50, windows=3)
    assert t3.windows == 3 and vc.dim(t3) == 24 and vc.fvconvert(t3, Xs[-1].T).shape == (8, 50)
    # dim(g) = 8 is no static + delta + delta-delta
    g8 = vc.BlockDiagGMMMap(*bdiag_model(1, 16, 2))
    with pytest.raises(vc.DimensionMismatch, match="delta-delta"):
        vc.BlockDiagTrajectoryGMMMap(g8, 10, windows=3)
    assert len(vc.BlockDiagTrajectoryGMMMap(g8, 10)) == 10 and vc.fvconvert(g8, np.zeros((8, 2))).shape == (8, 2)
    # any other window count
    for w in (0, 1, 4, -3):
        with pytest.raises(vc.VCMIError, match="windows"):
            vc.BlockDiagTrajectoryGMMMap(g, 50, windows=w)
    with pytest.raises(TypeError, match="windows"):
        vc.BlockDiagTrajectoryGMMMap(g, 50, windows=3.0)
    # the EM converter's constructor is unchanged: two windows
    assert vc.BlockDiagTrajectoryEMGMMMap(g, 50, em_iters=1).windows == 2
    with pytest.raises(TypeError):
        vc.BlockDiagTrajectoryEMGMMMap(g, 50, windows=3)


# ------------------------------------------------------------------------------------------------ 8. the point of the feature
def test_a_fitted_block_diag_model_over_three_windows_enters_trajectory_conversion_as_it_is(vc):
    """train_gmm(covariance_type="block_diag") on joint static + delta + delta-delta features (Dj = 24: static D = 4; M = 3, 4000
    frames: the generators of tests/test_gpu_traj_bdiag.py's fitted-model test) -> BlockDiagTrajectoryGMMMap(windows=3) straight
    from the result, against the restatement of the fitted numbers.  T = 70: a tile and six frames."""
    import torch
    from em_bdiag_restatement import bdiag_model, draw
    Dj, M, N, T = 24, 3, 4000, 70
    D = Dj // 6
    w0, mu0, cov0 = bdiag_model(101, Dj, M, sep=6.0)
    Z = draw(102, w0, mu0, cov0, N)
    r = vc.train_gmm(torch.from_numpy(np.ascontiguousarray(Z)).cuda().t(), n_components=M, n_init=1, init="kmeans", n_iter=30,
                     covariance_type="block_diag")
    model = (r["weights"], r["means"], r["covars"])
    static = np.cumsum(draw(103, w0, mu0, cov0, T)[:, :D], axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
    X = R.push_delta2(static)
    bt = R.PentaTrajectory(*model)
    gap, bound = bt.undecided(X)
    assert bt.D == D and np.all(bt.q > 0) and int(np.sum(~(gap > bound))) == 0, (gap.min(), bound.max())
    ref, cond, rho = bt.banded(X)
    g = vc.BlockDiagGMMMap(*model)
    t = vc.BlockDiagTrajectoryGMMMap(g, T, windows=3)
    assert vc.dim(t) == 3 * D
    y = vc.fvconvert(t, X.T)
    _check(y, ref.T, cond, rho, "fitted model against the restatement")
    _check(y, bt.dense(X).T, cond, rho, "fitted model against the explicit W")
