"""GPU: EM re-estimation of the trajectory over all mixtures (TrajectoryGMMMap(g, T, em_iters=n), csrc/traj_em.hip) against the
numpy restatement tests/traj_em_restatement.py.  The inputs and what they have to satisfy are checked on the CPU by
tests/test_traj_em_host.py; the references are computed once per case (traj_em_restatement.case_reference).

Tolerances.  Parity on the synthetic models 1e-9 relative: what tests/test_gpu_trajectory.py holds this file's solvers to each
other at; a 1e-13 perturbation of X moves the restatement's y by < 1e-12 (measured 0.6 .. 2.1e-13, test_traj_em_host.py):
three orders of margin.  On the trained model 1e-6,
test_gpu_trajectory.py's TOL.  Objective 1e-10 relative: a sum of T log-sum-exps of O(1e2) nats each in FP64.  Two library
paths that run the same kernels on the same bits: equal."""
import numpy as np
import pytest

import traj_em_restatement as R
from conftest import julia_model, load_golden, relerr

pytestmark = pytest.mark.gpu
TOL_SYNTH = 1e-9
TOL_FIXTURE = 1e-6
TOL_L = 1e-10
ITERS = (1, 2, 4)


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    m.set_devices([])
    yield m
    m.set_devices([])


def converter(vc, name, em_iters=0):
    (w, mu, sig), Xs = R.case_inputs(name)
    g = vc.GMMMap(*julia_model(w, mu, sig))
    return vc.TrajectoryGMMMap(g, max(len(x) for x in Xs), em_iters=em_iters), [np.asfortranarray(x.T) for x in Xs]


def test_setting_roundtrip_and_errors(vc):
    from voiceconversion_jl_amd import _lib
    t, Xs = converter(vc, "native-16")
    assert t.em_iters == 0 and len(t.em_history()) == 0
    t.em_iters = 3
    assert t.em_iters == 3 and len(t.em_history()) == 0           # nothing has run yet
    t.fvconvert_batch(Xs)
    t.em_iters = 1
    assert len(t.em_history()) == 3                                  # the length of the LAST call, not of the setting
    t.em_iters = 3
    assert _lib.lib.vcmi_traj_set_em(t._h, -1) == _lib.VCMI_ERR_ARG and t.em_iters == 3
    with pytest.raises(vc.VCMIError):
        t.em_iters = -2
    # the GV ascent reads one mixture per frame: with EM on, every convert entry refuses before anything runs
    D = 16
    tgv = vc.TrajectoryGVGMMMap(t, np.ones(D), np.eye(D))
    Y = np.empty((D, Xs[0].shape[1]), order="F")
    assert _lib.lib.vcmi_trajgv_convert(tgv._h, _lib.dptr(Xs[0]), Xs[0].shape[1], 2, 1e-5, _lib.dptr(Y)) == _lib.VCMI_ERR_ARG
    with pytest.raises(vc.VCMIError):
        tgv.fvconvert_batch(Xs, epochs=2)
    with pytest.raises(vc.VCMIError):
        vc.vc(tgv, np.zeros((2 * D + 1, 40)))
    t.em_iters = 0
    assert len(tgv.fvconvert_batch(Xs, epochs=2)) == len(Xs)
    # cond_loglik: wrong dimensions
    with pytest.raises(vc.DimensionMismatch):
        t.cond_loglik(np.zeros((2 * D - 2, 5)), np.zeros((D, 5)))
    with pytest.raises(vc.DimensionMismatch):
        t.cond_loglik(np.zeros((2 * D, 5)), np.zeros((D, 4)))
    with pytest.raises(vc.DimensionMismatch):
        t.cond_loglik(np.zeros((2 * D, 5)), np.zeros((D - 1, 5)))


def test_indefinite_precision_refuses_em_only(vc):
    """(Q_m + Q_m')/2 indefinite -- Q = diag(I, -I/4): no log-determinant, so EM cannot be switched on -- but W'QW =
    sum |y_t|^2 - sum |delta y_t|^2 / 4 is positive definite: with em_iters = 0 the model converts as it always did, to the
    bytes of a handle that was never configured, and a refused setter leaves it so."""
    from oracle import np_oracle as npo
    D, M, T = 12, 2, 9
    rng = np.random.default_rng(3)
    C = np.diag(np.r_[np.ones(D), -4.0 * np.ones(D)])                # conditional covariance of y (A = 0): indefinite
    Z = np.zeros((2 * D, 2 * D))
    sig = np.stack([np.block([[np.eye(2 * D), Z], [Z, C]])] * M)
    w, mu = np.array([0.4, 0.6]), rng.standard_normal((M, 4 * D))
    X = np.asfortranarray(rng.standard_normal((2 * D, T)))
    g = vc.GMMMap(*julia_model(w, mu, sig))
    never = vc.fvconvert(vc.TrajectoryGMMMap(g, T), X)
    assert relerr(never, npo.TrajectoryGMMMap(npo.GMMMap(w, mu, sig)).fvconvert(np.ascontiguousarray(X.T))[0].T) < TOL_FIXTURE
    with pytest.raises(vc.PosDefException):
        vc.TrajectoryGMMMap(g, T, em_iters=1)
    t = vc.TrajectoryGMMMap(g, T, em_iters=0)
    assert vc.fvconvert(t, X).tobytes() == never.tobytes()
    with pytest.raises(vc.PosDefException):
        t.em_iters = 2
    assert t.em_iters == 0
    assert vc.fvconvert(t, X).tobytes() == never.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(t.fvconvert_batch([X, X[:, :4]]), [never, vc.fvconvert(t, X[:, :4])]))
    with pytest.raises(vc.PosDefException):
        t.cond_loglik(X, np.zeros((D, T)))


def test_slices_do_not_change_the_result(vc):
    """The batch starts as one slice and is cut where an iteration's mixed-frame count takes the table past the cap.  With the
    cap lowered (test hook) to the model's matrices plus 40 / 5 blended ones, the 7- and 4-utterance batches are cut several
    times, down to single utterances that exceed it: the same bits and the same objective as the uncut run."""
    import ctypes as C
    from voiceconversion_jl_amd import _lib
    hook = _lib.lib.vcmi_debug_traj_em_cap
    hook.argtypes, hook.restype = [C.c_void_p, C.c_size_t], C.c_int
    times = _lib.lib.vcmi_debug_traj_em_times
    times.argtypes, times.restype = [C.c_void_p, C.c_int, C.POINTER(C.c_double)], C.c_int
    for name, extra in (("stencil-12", 40), ("native-20", 5), ("padded-13", 5)):
        t, Xs = converter(vc, name, em_iters=2)
        D, M = R.CASES[name][1], R.CASES[name][2]
        want, hwant = t.fvconvert_batch(Xs), t.em_history()
        Ds = {13: 16}.get(D, D)                                      # the dimension the solver runs in
        _lib.check(hook(t._h, 8 * (M + extra) * (2 * Ds) ** 2))
        out = (C.c_double * 8)()
        _lib.check(times(t._h, 1, out))
        got, hgot = t.fvconvert_batch(Xs), t.em_history()
        _lib.check(times(t._h, 0, out))
        _lib.check(hook(t._h, 0))
        assert out[7] > 2 * 1, out[7]                                # more slice-iterations than one slice's two
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        assert np.all(np.abs(hgot - hwant) <= 1e-12 * np.abs(hwant))


@pytest.mark.parametrize("name", R.OVERLAP)
def test_parity_with_the_restatement(vc, name):
    """y^n for n = 1, 2, 4 on models where every frame is a blend; the batch call equals the single call bit for bit and a
    repeated call gives the same bits.  Fails on a library without EM (y^1 is 5 .. 96 % of max |y| away from y^0).  The cases valu-* (2D > 96)
    take the one-workgroup-per-frame kernels by themselves, with the fallback solvers (window in LDS, and in HBM above D = 64)."""
    t, Xs = converter(vc, name)
    refs = R.case_reference(name)
    for n in ITERS:
        t.em_iters = n
        Ys = t.fvconvert_batch(Xs)
        for x, y, r in zip(Xs, Ys, refs):
            assert y.shape == (x.shape[0] // 2, x.shape[1])
            if r is not None:
                e = relerr(y, r["ys"][n].T)
                print(f"{name} T={x.shape[1]} n={n}: {e:.2e}")
                assert e < TOL_SYNTH
        assert np.array_equal(vc.fvconvert(t, Xs[0]), Ys[0])
        if n == 2:
            assert all(np.array_equal(a, b) for a, b in zip(t.fvconvert_batch(Xs), Ys))
            k = min(range(len(Xs)), key=lambda i: Xs[i].shape[1] or 1 << 30)        # the shortest non-empty one, alone
            assert np.array_equal(vc.fvconvert(t, Xs[k]), Ys[k])


def test_mfma_and_per_frame_kernels_agree(vc):
    """The MFMA E-step / gbar kernels against the one-workgroup-per-frame kernel (the path of 2D > 96) on the same input."""
    from voiceconversion_jl_amd import _lib
    t, Xs = converter(vc, "native-20", em_iters=2)
    Ya = t.fvconvert_batch(Xs)
    ha = t.em_history()
    _lib.debug_force(_lib.DBG_TRAJ_G_SCALAR)
    try:
        Yb = t.fvconvert_batch(Xs)
        hb = t.em_history()
    finally:
        _lib.debug_force(0)
    for a, b in zip(Ya, Yb):
        assert a.shape == b.shape and (a.size == 0 or relerr(a, b) < TOL_SYNTH)
    assert np.all(np.abs(ha - hb) <= TOL_L * np.abs(ha))


def test_parity_on_the_trained_model(vc, fixture_model):
    """Pure and mixed frames in one table: the first E-step has a handful of mixed frames (gaps 0.17 .. 22 nats), later ones
    none (every gap > 41 nats)."""
    _, X, r = R.fixture_reference()
    t = vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*fixture_model)), 100)
    Xj = np.asfortranarray(X.T)
    y0 = vc.fvconvert(t, Xj)
    assert relerr(y0, r["ys"][0].T) < TOL_FIXTURE
    for n in ITERS:
        t.em_iters = n
        y = vc.fvconvert(t, Xj)
        e = relerr(y, r["ys"][n].T)
        print(f"fixture n={n}: {e:.2e}; moved {relerr(y, y0):.2e} from the arg-max solution")
        assert e < TOL_FIXTURE
        h = t.em_history()
        print("fixture objective:", h, "restatement:", r["L"][:n])
        assert len(h) == n and np.all(np.isfinite(h)) and np.all(np.diff(h) >= 0.0)
        assert np.array_equal(t.fvconvert_batch([Xj, Xj[:, :37]])[0], y)


def test_unchanged_default(vc):
    """em_iters = 0, set explicitly or after a detour through EM, and a handle that was never configured: the same bytes."""
    for name in ("stencil-12", "padded-13", "peaked-20"):
        fresh, Xs = converter(vc, name)
        Ya = fresh.fvconvert_batch(Xs)
        zero, _ = converter(vc, name, em_iters=0)
        zero.em_iters = 0
        back, _ = converter(vc, name, em_iters=2)
        Yem = back.fvconvert_batch(Xs)
        back.em_iters = 0
        for a, b, c in zip(Ya, zero.fvconvert_batch(Xs), back.fvconvert_batch(Xs)):
            assert a.tobytes() == b.tobytes() == c.tobytes()
        if name != "peaked-20":
            assert not np.array_equal(Yem[0], Ya[0])
        assert len(Yem) == len(Xs) and len(back.em_history()) == 0      # the last call ran no iteration
        back.em_iters = 3
        assert len(back.em_history()) == 0                               # ... whatever the setting is now


@pytest.mark.parametrize("name", R.PEAKED)
def test_peaked_models_reproduce_the_argmax_solution(vc, name):
    """No frame is mixed (every gap > 100 nats): each frame keeps one mixture, the table is the model's own, and EM must
    return the arg-max solution and a constant objective."""
    t, Xs = converter(vc, name)
    Y0 = t.fvconvert_batch(Xs)
    t.em_iters = 3
    Y3 = t.fvconvert_batch(Xs)
    for a, b in zip(Y0, Y3):
        assert relerr(b, a) < 1e-12
    h = t.em_history()
    assert len(h) == 3 and np.all(np.isfinite(h)) and np.all(np.abs(h - h[0]) <= 1e-12 * np.abs(h[0]))
    want = sum(r["L"][0] for r in R.case_reference(name) if r is not None)
    assert abs(h[0] - want) <= TOL_L * abs(want)


@pytest.mark.parametrize("name", R.OVERLAP + ["peaked-12"])
def test_conditional_loglik(vc, name):
    """cond_loglik at the restatement's own y^n against its L[n], host and device entries; on the library's y^n it never
    falls (slack 1e-10 |L| for the rounding of the sum) and rises strictly in the first iteration of an overlapping model;
    em_history() is the objective of the intermediate results."""
    import torch
    t, Xs = converter(vc, name)
    refs = R.case_reference(name)
    for x, r in zip(Xs, refs):
        if r is None:
            assert t.cond_loglik(x, np.zeros((x.shape[0] // 2, 0))) == 0.0
            continue
        for n in (0, 1, 4):
            y = np.asfortranarray(r["ys"][n].T)
            L = t.cond_loglik(x, y)
            assert abs(L - r["L"][n]) <= TOL_L * abs(r["L"][n]), (n, L, r["L"][n])
            dx = torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t()
            dy = torch.from_numpy(np.ascontiguousarray(y.T)).cuda().t()
            Ld = t.cond_loglik(dx, dy)
            assert Ld.is_cuda and float(Ld.cpu()[0]) == L
    Ys = [t.fvconvert_batch(Xs)]
    for n in range(1, 5):
        t.em_iters = n
        Ys.append(t.fvconvert_batch(Xs))
    hist = t.em_history()                                            # of the em_iters = 4 call
    t.em_iters = 0
    Ls = np.array([[t.cond_loglik(x, y) for x, y in zip(Xs, Y)] for Y in Ys])       # [n][utterance]
    print(name, "L per iteration:", Ls.sum(axis=1))
    assert np.all(np.diff(Ls, axis=0) >= -1e-10 * np.abs(Ls[:-1]))
    if name in R.OVERLAP:
        live = np.array([x.shape[1] > 0 for x in Xs])
        assert np.all(Ls[1][live] > Ls[0][live])                     # (the restatement's smallest first step is 1e-5 relative)
    assert np.all(np.abs(hist - Ls[:4].sum(axis=1)) <= 1e-12 * np.abs(hist))


def test_device_group_picks_up_a_later_setting(vc):
    """em_iters set AFTER a batch call that made the replicas of a device group (one device listed twice) still takes effect."""
    t, Xs = converter(vc, "native-16")
    (w, mu, sig), _ = R.case_inputs("native-16")
    refs = R.case_reference("native-16")
    batch = [Xs[i % 2] for i in range(10)]
    vc.set_devices([0, 0])
    try:
        Y0 = t.fvconvert_batch(batch)
        t.em_iters = 2
        Y2 = t.fvconvert_batch(batch)
        h2 = t.em_history()
    finally:
        vc.set_devices([])
    one = t.fvconvert_batch(batch)
    for i, (a, b, c) in enumerate(zip(Y0, Y2, one)):
        assert relerr(a, refs[i % 2]["ys"][0].T) < TOL_FIXTURE and relerr(b, refs[i % 2]["ys"][2].T) < TOL_SYNTH
        assert np.array_equal(b, c)
    want = 5 * sum(np.array(r["L"][:2]) for r in refs)
    assert np.all(np.abs(h2 - want) <= TOL_L * np.abs(want))
    assert np.all(np.abs(t.em_history() - want) <= TOL_L * np.abs(want))


def test_vc_runs_em_per_chunk(vc, fixture_model):
    """vc(t30, fm) with EM on = chunk-wise fvconvert with EM on: host matrix, device tensor, and static input (delta=True)."""
    import torch
    z = load_golden("trajectory_fixture_model.npz")
    g = vc.GMMMap(*julia_model(*fixture_model))
    fm = np.asfortranarray(z["vc_fm"].T)                              # (2D+1, T)
    T, L, D = fm.shape[1], 30, 20

    def chunkwise(X):
        tc = vc.TrajectoryGMMMap(g, L, em_iters=2)
        return np.concatenate([vc.fvconvert(tc, np.asfortranarray(X[:, b:b + L])) for b in range(0, T, L)], axis=1)

    want = chunkwise(fm[1:])
    plain = vc.vc(vc.TrajectoryGMMMap(g, L), fm)
    out = vc.vc(vc.TrajectoryGMMMap(g, L, em_iters=2), fm)
    assert out.shape == (D + 1, T) and np.array_equal(out[0], fm[0]) and np.array_equal(out[1:], want)
    assert relerr(out[1:], plain[1:]) > 1e-3                          # EM moved the trajectory
    dev = vc.vc(vc.TrajectoryGMMMap(g, L, em_iters=2), torch.from_numpy(np.ascontiguousarray(fm.T)).cuda().t())
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), out)
    static = np.asfortranarray(fm[:D + 1])
    wants = chunkwise(vc.push_delta(np.asfortranarray(static[1:])))
    outs = vc.vc(vc.TrajectoryGMMMap(g, L, em_iters=2), static, delta=True)
    assert np.array_equal(outs[0], static[0]) and np.array_equal(outs[1:], wants)
    devs = vc.vc(vc.TrajectoryGMMMap(g, L, em_iters=2), torch.from_numpy(np.ascontiguousarray(static.T)).cuda().t(), delta=True)
    assert np.array_equal(devs.cpu().numpy(), outs)
