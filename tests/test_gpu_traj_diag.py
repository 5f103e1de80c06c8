"""GPU: TrajectoryGMMMap with diagonal conditional precisions (precision="diag": vcmi_traj_set_precision, csrc/traj_diag.hip)
against the numpy restatement tests/traj_diag_restatement.py.

Tolerance: relerr < 64 cond 2^-53, cond the largest condition number of the tridiagonal systems of that input as the restatement
reports it -- both sides are FP64 and the Thomas recurrence is backward stable on these strictly diagonally dominant matrices.
Models and frames are those of tests/test_gpu_trajectory.py::test_vs_oracle_batch (synth_model(.., lam_lo=1e-3), scaled
cumulative sums), for its reason: the arg-max is far from ties, so both sides take the same mixture sequence."""
import functools

import numpy as np
import pytest

import traj_diag_restatement as R
from conftest import julia_model, relerr

pytestmark = pytest.mark.gpu
TOL_ORACLE = 1e-6                  # tests/test_gpu_trajectory.py against the C oracle


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


@functools.lru_cache(maxsize=None)
def _case(D, M, Ts):
    """model, utterances (T,2D) and their restated trajectories with the condition numbers: made once, never written to"""
    model, Xs = R.make_case(D, M, list(Ts))
    dt = R.DiagTrajectory(*model)
    return model, Xs, [dt.tridiag(X) for X in Xs], dt


def _conv(vc, model, T, **kw):
    return vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*model)), T, **kw)


def _check(y, ref, cond, what=""):
    err = relerr(y, ref) if ref.size else 0.0
    print(f"{what}: relerr {err:.3e}  cond {cond:.3f}  bound {R.tolerance(cond):.3e}")
    assert y.shape == ref.shape
    assert err < R.tolerance(cond), (what, err, R.tolerance(cond))


# ------------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("D,M,Ts", [(D, M, tuple(Ts)) for D, M, Ts in R.SHAPES])
def test_vs_restatement_batch(vc, D, M, Ts):
    """D = 40: two slabs, the second with 8 live lanes; T = 1..5: chains of length 0, 1, 2, 3 and the stencil without neighbours;
    D = 7: one partial slab; D = 33: one lane past a slab, both parities of T; D = 59: 2D > 96 puts g_t on the one-workgroup-
    per-frame kernel, and the solver for D >= 47 is never entered.  An empty utterance rides in every batch."""
    model, Xs, refs, _ = _case(D, M, Ts)
    t = _conv(vc, model, max(Ts), precision="diag")
    assert t.precision == "diag"
    batch = [X.T for X in Xs[:1]] + [np.zeros((2 * D, 0), order="F")] + [X.T for X in Xs[1:]]
    Ys = t.fvconvert_batch(batch)
    assert Ys[1].shape == (D, 0)
    Ys = Ys[:1] + Ys[2:]
    for X, y, (ref, cond) in zip(Xs, Ys, refs):
        _check(y, ref.T, cond, f"D={D} T={X.shape[0]}")
    # batch == single, bit for bit
    for X, y in zip(Xs, Ys):
        assert np.array_equal(vc.fvconvert(t, X.T), y)


# ------------------------------------------------------------------------- 2. a conditional covariance that IS diagonal
def test_diagonal_by_construction_ties_both_modes_to_the_oracle(vc):
    """Syx = A Sxx, Syy = diag(c) + A Sxx A': the conditional covariance is diag(c) up to rounding, so the diagonal mode, the
    full mode and the C oracle's TrajectoryGMMMap solve the same problem."""
    from oracle import c_oracle as co
    D, M, T = 12, 4, 50
    model = R.diagonal_conditional_model(71, D, M)
    dt = R.DiagTrajectory(*model)
    assert max(np.max(np.abs(C - np.diag(np.diag(C)))) for C in dt.C) < 1e-13
    X = R.smooth_frames(np.random.default_rng(3), *model, T, D)
    t = _conv(vc, model, T)
    yfull = vc.fvconvert(t, X.T)
    t.precision = "diag"
    ydiag = vc.fvconvert(t, X.T)
    yref = co.TrajectoryGMMMap(co.GMMMap(*model)).fvconvert(X)[0].T
    print("diag vs oracle", relerr(ydiag, yref), "full vs oracle", relerr(yfull, yref), "diag vs full", relerr(ydiag, yfull))
    assert relerr(ydiag, yref) < TOL_ORACLE and relerr(yfull, yref) < TOL_ORACLE and relerr(ydiag, yfull) < TOL_ORACLE
    ref, cond = dt.tridiag(X)
    _check(ydiag, ref.T, cond, "diagonal by construction")


# ------------------------------------------------------------------------------------------------ 3. ill-conditioned systems
def test_ill_conditioned_tridiagonals(vc):
    """delta precisions ~1e8 x the static ones: the matrices approach the singular second-difference operator"""
    D, M, T = 12, 4, 50
    model = R.ill_conditioned_model(81, D, M)
    dt = R.DiagTrajectory(*model)
    ratio = float(np.median(dt.q[:, D:] / dt.q[:, :D]))
    assert 1e7 < ratio < 1e9, ratio
    X = R.smooth_frames(np.random.default_rng(4), *model, T, D)
    ref, cond = dt.tridiag(X)
    assert cond > 1e3 and R.tolerance(cond) < 1e-6, cond          # harder than the other cases, and not vacuous
    t = _conv(vc, model, T, precision="diag")
    _check(vc.fvconvert(t, X.T), ref.T, cond, f"p_d/p_s = {ratio:.2e}")


# ------------------------------------------------------------------------------------------------ 4. bits
def test_toggles_and_a_second_stream_leave_the_bits_alone(vc):
    import torch
    D, M, Ts = 12, 4, (1, 2, 3, 4, 5, 50)
    model, Xs, _, _ = _case(D, M, Ts)
    batch = [X.T for X in Xs]
    t = _conv(vc, model, 50)
    full0 = t.fvconvert_batch(batch)
    t.precision = "diag"
    diag0 = t.fvconvert_batch(batch)
    assert not np.array_equal(diag0[-1], full0[-1])
    fm = np.asfortranarray(np.vstack([np.arange(50.0)[None, :], Xs[-1].T]))
    dfm = torch.from_numpy(np.ascontiguousarray(fm.T)).cuda().t()
    dev0 = vc.vc(t, dfm).cpu().numpy()
    assert np.array_equal(dev0[1:], diag0[-1])
    for kind in ("full", "diag", "full", "diag"):
        t.precision = kind
        assert t.precision == kind
        got = t.fvconvert_batch(batch)
        assert all(np.array_equal(a, b) for a, b in zip(got, full0 if kind == "full" else diag0)), kind
        # another size in between (through the batch entry: a single call would leave len(t), the chunk length of vc, at 4)
        assert np.array_equal(t.fvconvert_batch(batch[2:4])[1], (full0 if kind == "full" else diag0)[3])
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        dev1 = vc.vc(t, dfm)
    s1.synchronize()
    assert np.array_equal(dev1.cpu().numpy(), dev0)


# ------------------------------------------------------------------------------------------------ 5. the vc surface
def _vc_inputs():
    D, M, T, L = 12, 4, 100, 30
    model, Xs, _, dt = _case(D, M, (T,))
    power = np.linspace(-3.0, 2.0, T)
    static = np.concatenate([power[:, None], Xs[0][:, :D]], axis=1)          # (T, D+1)
    full = np.concatenate([power[:, None], Xs[0]], axis=1)                    # (T, 2D+1)
    return D, M, T, L, model, dt, static, full


def test_vc_surface_against_the_restatement_chunk_by_chunk(vc):
    import torch
    from oracle import np_oracle as npo
    D, M, T, L, model, dt, static, full = _vc_inputs()
    want, cond = dt.vc(full, L)                                               # chunks 30, 30, 30 and a tail of 10
    fresh = lambda: _conv(vc, model, L, precision="diag")                     # noqa: E731  (vc leaves len(c) at the tail's length)
    out = vc.vc(fresh(), np.asfortranarray(full.T))
    assert np.array_equal(out[0], full[:, 0])
    _check(out[1:], want[:, 1:].T, cond, "vc(t, fm)")
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
    _check(outf[1:], wantf.T, cond, "vc with VarianceScaling")
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
        w2, c2 = dt.vc(np.concatenate([static[:37, :1], npo.push_delta(static[:37, 1:])], axis=1), L)
        if pf is None:
            _check(outs[0][1:], want[:, 1:].T, cond, "vc_batch[0]")
            _check(outs[2][1:], w2[:, 1:].T, c2, "vc_batch[2]")
        else:
            _check(outs[0][1:], wantf.T, cond, "vc_batch[0] filtered")
            _check(outs[2][1:], npo.variance_scaling(w2[:, 1:], s2).T, c2, "vc_batch[2] filtered")


# ------------------------------------------------------------------------------------------------ 6. what is refused
def test_refusals_leave_a_working_handle(vc):
    D, M, Ts = 12, 4, (1, 2, 3, 4, 5, 50)
    model, Xs, refs, _ = _case(D, M, Ts)
    X = np.asfortranarray(Xs[-1].T)

    def still_converts(t, kind):
        assert t.precision == kind
        if kind == "diag":
            _check(vc.fvconvert(t, X), refs[-1][0].T, refs[-1][1], "after a refusal")
        else:
            assert vc.fvconvert(t, X).shape == (D, 50)

    # EM and the diagonal model, in either order
    with pytest.raises(vc.VCMIError, match="EM"):
        _conv(vc, model, 50, em_iters=2, precision="diag")
    t = _conv(vc, model, 50, em_iters=2)
    with pytest.raises(vc.VCMIError, match="EM"):
        t.precision = "diag"
    assert t.em_iters == 2
    still_converts(t, "full")
    t = _conv(vc, model, 50, precision="diag")
    with pytest.raises(vc.VCMIError, match="diagonal"):
        t.em_iters = 2
    assert t.em_iters == 0
    still_converts(t, "diag")
    # a GV converter over a diagonal handle
    muv = np.var(refs[-1][0], axis=0, ddof=1) * 1.2
    tgv = vc.TrajectoryGVGMMMap(t, muv, np.diag(muv ** 2 * 0.1))
    with pytest.raises(vc.VCMIError, match="diagonal"):
        vc.fvconvert(tgv, X, epochs=3)
    fm = np.asfortranarray(np.vstack([np.ones((1, 50)), X]))
    with pytest.raises(vc.VCMIError, match="diagonal"):
        vc.vc(tgv, fm)
    with pytest.raises(vc.VCMIError, match="diagonal"):
        tgv._vc(fm, vc.VarianceScaling(muv))
    with pytest.raises(vc.VCMIError, match="diagonal"):
        vc.vc_batch(tgv, [fm, fm])
    still_converts(t, "diag")
    t.precision = "full"
    assert vc.fvconvert(tgv, X, epochs=3).shape == (D, 50)               # ... and over the same handle in full mode it runs
    t.precision = "diag"
    # an unknown kind
    from voiceconversion_jl_amd import _lib
    with pytest.raises(vc.VCMIError, match="unknown kind"):
        t.precision = "banded"
    assert _lib.lib.vcmi_traj_set_precision(t._h, 2) == _lib.VCMI_ERR_ARG
    assert _lib.lib.vcmi_traj_set_precision(None, 1) == _lib.VCMI_ERR_ARG and _lib.lib.vcmi_traj_get_precision(None) == -1
    still_converts(t, "diag")


def test_not_positive_conditional_variance(vc):
    """the joint covariance of tests/test_gpu_trajectory.py::test_not_positive_definite_normal_matrix: conditional variances
    1 - 4 = -3 -> PosDefException at the switch, and the handle stays in full mode"""
    D, M = 12, 2
    I = np.eye(2 * D)
    sig = np.stack([np.block([[I, 2.0 * I], [2.0 * I, I]])] * M)
    model = (np.array([0.5, 0.5]), np.random.default_rng(3).standard_normal((M, 4 * D)), sig)
    t = _conv(vc, model, 9)
    with pytest.raises(vc.PosDefException):
        t.precision = "diag"
    assert t.precision == "full"


# ------------------------------------------------------------------------------------------------ 7. a device group
def test_device_group_replicas_convert_in_diagonal_mode(vc):
    """the group [0, 0] of tests/test_gpu_group.py: from 8 utterances on the batch is split over two worker threads, the second
    of which converts on a replica that has to receive the setting and its own diagonal model"""
    D, M = 12, 4
    model, _, _, dt = _case(D, M, (1, 2, 3, 4, 5, 50))
    rng = np.random.default_rng(8)
    Xs = [R.smooth_frames(rng, *model, T, D) for T in [50, 31, 2, 77, 50, 50, 9, 64, 13, 40, 50]]
    batch = [np.asfortranarray(X.T) for X in Xs]
    t = _conv(vc, model, 50, precision="diag")
    vc.set_devices([])
    one = t.fvconvert_batch(batch)
    try:
        vc.set_devices([0, 0])
        two = t.fvconvert_batch(batch)
        t.precision = "full"
        full = t.fvconvert_batch(batch)
        t.precision = "diag"
        again = t.fvconvert_batch(batch)
    finally:
        vc.set_devices([])
    for a, b, c in zip(one, two, again):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert not np.array_equal(full[3], one[3])
    ref, cond = dt.tridiag(Xs[3])
    _check(two[3], ref.T, cond, "group member")
