"""GPU: BlockDiagTrajectoryGMMMap -- trajectory conversion straight from a cross-diagonal model (vcmi_traj_create_bdiag: the fused
arg-max + g_t pass of csrc/gmmmap_bdiag.hip, mode 3, and the tridiagonal solver of csrc/traj_diag.hip) -- against the numpy
restatement tests/traj_bdiag_restatement.py and against the detour through the expanded model.

Tolerance: relerr < 64 cond rho 2^-53 (twice that between the two device paths), cond the largest condition number of the
tridiagonal systems of the input and rho the cancellation the centred g can carry into the right-hand side, both as the
restatement reports them; derived in its docstring.  tests/test_traj_bdiag_restatement_host.py asserts for every input used here
that every q > 0 and that no frame's arg-max is within rounding of a tie, so both sides take the same mixture sequence."""
import functools
import gc

import numpy as np
import pytest

import traj_bdiag_restatement as R
import traj_diag_restatement as DR
from conftest import relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


@functools.lru_cache(maxsize=None)
def _case(D, M, Ts, swap=False):
    """model, utterances (T,2D), their restated trajectories (Y, cond, rho) and the restatement: made once, never written to"""
    model, Xs = R.make_case(D, M, list(Ts), swap)
    bt = R.BdiagTrajectory(*model, swap)
    return model, Xs, [bt.tridiag(X) for X in Xs], bt


def _conv(vc, model, T, swap=False):
    return vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(*model, swap=swap), T)


def _detour(vc, model, T):
    w, mu, cov = model
    return vc.TrajectoryGMMMap(vc.GMMMap(w, mu, vc.expand_block_diag(cov)), T, precision="diag")


def _check(y, ref, cond, rho, what="", factor=1.0):
    err = relerr(y, ref) if ref.size else 0.0
    bound = factor * DR.tolerance(cond) * rho
    print(f"{what}: relerr {err:.3e}  cond {cond:.3f}  rho {rho:.3f}  bound {bound:.3e}")
    assert y.shape == ref.shape
    assert err < bound, (what, err, bound)


# ------------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("D,M,Ts", [(D, M, tuple(Ts)) for D, M, Ts in R.SHAPES])
def test_vs_restatement_batch(vc, D, M, Ts):
    """D = 40, M = 8: 2D = 80 features, five 64-frame tiles with a partial last one; T = 1..5: tiles of one to five frames and
    the stencil without neighbours; D = 7: 2D = 14 is padded to 16 in the tables; D = 33: one lane past a solver slab, T = 64 and
    65 fill a tile and step one frame past it; D = 64: the limit 2D = 128; M = 256 at 2D = 8: the kernel's 32-frame tiles (the
    log-densities of 256 mixtures do not fit LDS beside 64 frames), 16 mixtures per part of the first-maximum reduction, 13
    distinct mixtures in the utterance (per-lane gather); D = 40, M = 64: the benchmark's model,
    three tiles.  An empty utterance rides in every batch."""
    model, Xs, refs, _ = _case(D, M, Ts)
    t = _conv(vc, model, max(Ts))
    assert t.precision == "diag" and vc.dim(t) == 2 * D and vc.ncomponents(t) == M and len(t) == max(Ts)
    batch = [X.T for X in Xs[:1]] + [np.zeros((2 * D, 0), order="F")] + [X.T for X in Xs[1:]]
    Ys = t.fvconvert_batch(batch)
    assert Ys[1].shape == (D, 0)
    Ys = Ys[:1] + Ys[2:]
    for X, y, (ref, cond, rho) in zip(Xs, Ys, refs):
        _check(y, ref.T, cond, rho, f"D={D} M={M} T={X.shape[0]}")
    # batch == single, bit for bit
    for X, y in zip(Xs, Ys):
        assert np.array_equal(vc.fvconvert(t, X.T), y)


# ------------------------------------------------------------------------------------------------ 2. against the detour
@pytest.mark.parametrize("D,M,Ts", [(12, 4, (1, 2, 3, 4, 5, 50)), (40, 64, (130,))])
def test_vs_the_detour_through_the_expanded_model(vc, D, M, Ts):
    """TrajectoryGMMMap(GMMMap(w, mu, expand_block_diag(covars)), T, precision="diag"), both sides on the device, within twice
    the tolerance (each is within one of the exact solution)"""
    model, Xs, refs, _ = _case(D, M, Ts)
    batch = [X.T for X in Xs]
    new = _conv(vc, model, max(Ts)).fvconvert_batch(batch)
    old = _detour(vc, model, max(Ts)).fvconvert_batch(batch)
    for X, a, b, (_, cond, rho) in zip(Xs, new, old, refs):
        _check(a, b, cond, rho, f"D={D} T={X.shape[0]} against the detour", factor=2.0)


# ------------------------------------------------------------------------------------------------ 3. the first maximum
def test_first_maximum_rule_and_a_mixture_without_weight(vc):
    """D = 3, M = 3, T = 10: mixtures 1 and 2 have bit-identical weights and source sides (their log-densities are the same
    number) and different target sides: the result is the restatement's with mhat = the lower index.  Mixture 3 sits on the
    frames' own mean and has weight 0: never chosen."""
    model, X = R.tie_case()
    bt = R.BdiagTrajectory(*model)
    g = vc.BlockDiagGMMMap(*model)
    assert np.all(vc.predict(g.px, X.T) == 1)
    y = vc.fvconvert(vc.BlockDiagTrajectoryGMMMap(g, 10), X.T)
    ref, cond, rho = bt.tridiag(X, mhat=np.ones(10, dtype=np.int64))
    _check(y, ref.T, cond, rho, "tie -> mixture 1")
    other = bt.tridiag(X, mhat=np.full(10, 2))[0]
    assert relerr(y, other.T) > 1e-3


# ------------------------------------------------------------------------------------------------ 4. swap
def test_swap(vc):
    """the (12, 4) shape with the halves of the model exchanged: source = rows 2D .. 4D-1"""
    D, M, Ts = 12, 4, (1, 2, 3, 4, 5, 50)
    model, Xs, refs, _ = _case(D, M, Ts, True)
    t = _conv(vc, model, 50, swap=True)
    for X, y, (ref, cond, rho) in zip(Xs, t.fvconvert_batch([X.T for X in Xs]), refs):
        _check(y, ref.T, cond, rho, f"swap T={X.shape[0]}")
    unswapped = vc.fvconvert(_conv(vc, model, 50), Xs[-1].T)
    assert relerr(unswapped, refs[-1][0].T) > 1e-3


# ------------------------------------------------------------------------------------------------ 5. the vc surface
def _vc_inputs():
    D, M, (T,) = R.VC_CASE
    L = 30
    model, Xs, _, bt = _case(D, M, (T,))
    power = np.linspace(-3.0, 2.0, T)
    static = np.concatenate([power[:, None], Xs[0][:, :D]], axis=1)          # (T, D+1)
    full = np.concatenate([power[:, None], Xs[0]], axis=1)                    # (T, 2D+1)
    return D, M, T, L, model, bt, static, full


def test_vc_surface_against_the_restatement_chunk_by_chunk(vc):
    """D = 12, M = 4, T = 100 in chunks of len(c) = 30: three whole chunks and a tail of 10"""
    import torch
    from oracle import np_oracle as npo
    D, M, T, L, model, bt, static, full = _vc_inputs()
    want, cond, rho = bt.vc(full, L)
    fresh = lambda: _conv(vc, model, L)                                       # noqa: E731  (vc leaves len(c) at the tail's length)
    c = fresh()
    out = vc.vc(c, np.asfortranarray(full.T))
    assert np.array_equal(out[0], full[:, 0]) and len(c) == 10
    _check(out[1:], want[:, 1:].T, cond, rho, "vc(t, fm)")
    # delta=True: deltas over the whole matrix first -- the frames the restatement was given
    assert np.array_equal(npo.push_delta(static[:, 1:]), full[:, 1:])
    outs = vc.vc(fresh(), np.asfortranarray(static.T), delta=True)
    assert np.array_equal(outs, out)
    # a VarianceScaling post-filter over the whole converted utterance
    s2 = np.var(want[:, 1:], axis=0, ddof=1) * np.linspace(0.5, 2.0, D)
    vs = vc.VarianceScaling(s2)
    wantf = npo.variance_scaling(want[:, 1:], s2)
    outf = vc.vc(fresh(), np.asfortranarray(static.T), postfilter=vs, delta=True)
    assert np.array_equal(outf[0], full[:, 0])
    _check(outf[1:], wantf.T, cond, rho, "vc with VarianceScaling")
    assert np.array_equal(vc.vc(fresh(), np.asfortranarray(full.T), postfilter=vs), outf)
    # a device tensor
    dfm = torch.from_numpy(static.copy()).cuda().t()
    outd = vc.vc(fresh(), dfm, delta=True)
    assert outd.is_cuda and np.array_equal(outd.cpu().numpy(), out)
    # vc_batch of three utterances, one of them empty: the restatement, and the single call bit for bit
    fms = [np.asfortranarray(static.T), np.zeros((D + 1, 0), order="F"), np.asfortranarray(static[:37].T)]
    for pf in (None, vs):
        c = fresh()
        outs = vc.vc_batch(c, fms, postfilter=pf, delta=True)
        assert len(c) == L and outs[1].shape == (D + 1, 0)
        for u in (0, 2):
            assert np.array_equal(outs[u], vc.vc(fresh(), fms[u], postfilter=pf, delta=True)), (pf is not None, u)
        w2, c2, r2 = bt.vc(np.concatenate([static[:37, :1], npo.push_delta(static[:37, 1:])], axis=1), L)
        if pf is None:
            _check(outs[0][1:], want[:, 1:].T, cond, rho, "vc_batch[0]")
            _check(outs[2][1:], w2[:, 1:].T, c2, r2, "vc_batch[2]")
        else:
            _check(outs[0][1:], wantf.T, cond, rho, "vc_batch[0] filtered")
            _check(outs[2][1:], npo.variance_scaling(w2[:, 1:], s2).T, c2, r2, "vc_batch[2] filtered")


# ------------------------------------------------------------------------------------------------ 6. bits
def test_repeats_a_second_stream_and_other_converters_leave_the_bits_alone(vc):
    """D = 12, M = 4, T = 1..50; the other converters in between: the detour on the same frames, a cross-diagonal converter of
    another shape (D = 7), and the frame-by-frame entry of the same BlockDiagGMMMap"""
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
    other_model, other_Xs, _, _ = _case(7, 2, (30, 2))
    others = [lambda: _detour(vc, model, 50).fvconvert_batch(batch),
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
    D, M, Ts = 12, 4, (1, 2, 3, 4, 5, 50)
    model, Xs, refs, _ = _case(D, M, Ts)
    X = np.asfortranarray(Xs[-1].T)
    Y = np.asfortranarray(refs[-1][0].T)
    t = _conv(vc, model, 50)

    def still_converts():
        assert t.precision == "diag" and t.em_iters == 0
        _check(vc.fvconvert(t, X), refs[-1][0].T, refs[-1][1], refs[-1][2], "after a refusal")

    with pytest.raises(vc.VCMIError, match="diagonal"):
        t.em_iters = 1
    still_converts()
    t.em_iters = 0                                                        # (switching it off is no request for EM)
    with pytest.raises(vc.VCMIError, match="cross-diagonal"):
        t.precision = "full"
    still_converts()
    t.precision = "diag"
    with pytest.raises(vc.VCMIError, match="cross-diagonal"):
        t.cond_loglik(X, Y)
    import torch
    dX, dY = (torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t() for a in (X, Y))
    with pytest.raises(vc.VCMIError, match="cross-diagonal"):
        t.cond_loglik(dX, dY)
    still_converts()
    # a GV converter over it: made, and refused at every convert entry
    muv = np.var(refs[-1][0], axis=0, ddof=1) * 1.2
    tgv = vc.TrajectoryGVGMMMap(t, muv, np.diag(muv ** 2 * 0.1))
    fm = np.asfortranarray(np.vstack([np.ones((1, 50)), X]))
    with pytest.raises(vc.VCMIError, match="diagonal"):
        vc.fvconvert(tgv, X, epochs=3)
    with pytest.raises(vc.VCMIError, match="diagonal"):
        vc.vc(tgv, fm)
    with pytest.raises(vc.VCMIError, match="diagonal"):
        tgv._vc(fm, vc.VarianceScaling(muv))
    with pytest.raises(vc.VCMIError, match="diagonal"):
        vc.vc_batch(tgv, [fm, fm])
    still_converts()


def test_constructor_refusals(vc):
    from em_bdiag_restatement import bdiag_model
    # odd dim(g): a joint dimension of 6 gives 3 features, which are no static + delta pairs
    g3 = vc.BlockDiagGMMMap(*bdiag_model(1, 6, 2))
    with pytest.raises(vc.DimensionMismatch, match="even"):
        vc.BlockDiagTrajectoryGMMMap(g3, 10)
    assert vc.fvconvert(g3, np.zeros((3, 2))).shape == (3, 2)
    # X with the wrong rows
    model, Xs, _, _ = _case(7, 2, (30, 2))
    t = _conv(vc, model, 30)
    for rows in (13, 15, 7):
        with pytest.raises(vc.DimensionMismatch):
            vc.fvconvert(t, np.zeros((rows, 5), order="F"))
        with pytest.raises(vc.DimensionMismatch):
            t.fvconvert_batch([Xs[0].T, np.zeros((rows, 5), order="F")])
    with pytest.raises(vc.DimensionMismatch):
        vc.vc(t, np.zeros((14, 5), order="F"))
    assert vc.fvconvert(t, Xs[1].T).shape == (7, 2)
    # anything but a BlockDiagGMMMap; and TrajectoryGMMMap still sends a BlockDiagGMMMap away, now with both ways named
    w, mu, cov = model
    with pytest.raises(TypeError, match="BlockDiagGMMMap"):
        vc.BlockDiagTrajectoryGMMMap(vc.GMMMap(w, mu, vc.expand_block_diag(cov)), 30)
    with pytest.raises(TypeError, match="expand_block_diag.*BlockDiagTrajectoryGMMMap"):
        vc.TrajectoryGMMMap(t.gmmmap, 30)
    # a VALID pair whose conditional variance rounds below zero (tests/c/traj_bdiag_prepare_check.cpp): the model converts frame
    # by frame, the trajectory converter names the pair
    bad = cov.copy(order="F")
    vx, vy, c = (float.fromhex(s) for s in ("0x1.40c25bc0b494dp+1", "0x1.ce0f24a25593fp-1", "0x1.80faec4f29850p+0"))
    bad[5, 1], bad[14 + 5, 1], bad[28 + 5, 1] = vx, vy, c
    gb = vc.BlockDiagGMMMap(w, mu, bad)
    assert vc.fvconvert(gb, Xs[1].T).shape == (14, 2)
    with pytest.raises(vc.PosDefException, match=r"pair \(6,2\)"):
        vc.BlockDiagTrajectoryGMMMap(gb, 30)
    assert vc.fvconvert(gb, Xs[1].T).shape == (14, 2)


# ------------------------------------------------------------------------------------------------ 8. lifetime
def test_the_converter_keeps_its_model_alive(vc):
    """D = 7, M = 2: the last user reference to the BlockDiagGMMMap is dropped before the first conversion"""
    model, Xs, refs, _ = _case(7, 2, (30, 2))
    g = vc.BlockDiagGMMMap(*model)
    t = vc.BlockDiagTrajectoryGMMMap(g, 30)
    del g
    gc.collect()
    vc.BlockDiagGMMMap(*_case(12, 4, (1, 2, 3, 4, 5, 50))[0])              # (an allocation that could take a freed table's place)
    _check(vc.fvconvert(t, Xs[0].T), refs[0][0].T, refs[0][1], refs[0][2], "after del g")


# ------------------------------------------------------------------------------------------------ 9. the point of the feature
def test_a_fitted_block_diag_model_enters_trajectory_conversion_as_it_is(vc):
    """train_gmm(covariance_type="block_diag") on joint static+delta features (Dj = 16: static D = 4; M = 3, 4000 frames: the
    generators of tests/test_gpu_gmmmap_bdiag.py's fitted-model test) -> BlockDiagTrajectoryGMMMap straight from the result,
    against the detour on the same fit and against the restatement of the fitted numbers.  T = 70: a tile and six frames."""
    import torch
    from em_bdiag_restatement import bdiag_model, draw
    from oracle import np_oracle as npo
    Dj, M, N, T = 16, 3, 4000, 70
    D = Dj // 4
    w0, mu0, cov0 = bdiag_model(101, Dj, M, sep=6.0)
    Z = draw(102, w0, mu0, cov0, N)
    r = vc.train_gmm(torch.from_numpy(np.ascontiguousarray(Z)).cuda().t(), n_components=M, n_init=1, init="kmeans", n_iter=30,
                     covariance_type="block_diag")
    model = (r["weights"], r["means"], r["covars"])
    static = np.cumsum(draw(103, w0, mu0, cov0, T)[:, :D], axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
    X = npo.push_delta(static)
    bt = R.BdiagTrajectory(*model)
    gap, bound = bt.undecided(X)
    assert np.all(bt.q > 0) and int(np.sum(~(gap > bound))) == 0, (gap.min(), bound.max())
    ref, cond, rho = bt.tridiag(X)
    g = vc.BlockDiagGMMMap(*model)
    y = vc.fvconvert(vc.BlockDiagTrajectoryGMMMap(g, T), X.T)
    _check(y, ref.T, cond, rho, "fitted model against the restatement")
    _check(y, vc.fvconvert(_detour(vc, model, T), X.T), cond, rho, "fitted model against the detour", factor=2.0)
