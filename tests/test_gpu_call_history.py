"""GPU: results must not depend on earlier calls, sizes or streams ("State that outlives a call").

Every other GPU test builds a handle, calls it once and compares with the oracle.  Here a SEQUENCE of calls runs on shared
handles and shared thread-local scratch (tests/call_history.py: `play`), and every step is held to

  * bit equality with the same single call in the fresh state -- a new thread and a new handle (`fresh`): the README's
    "identical inputs give identical bits whatever ran before";
  * the oracle, at the bar the entry already has elsewhere in the suite (so that "both wrong alike" is excluded):
    frame_relerr < 1e-9 for fvconvert, exact for predict and DTW, 1e-9 for posteriors and E-step statistics
    (test_gpu_estep.py), 1e-6 behind the trajectory solve, 1e-12 (times max(1, max |log sp|) per frame, the form of
    test_gpu_mgc.py) for the mel-cepstral transforms against tests/mgc_restatement.py.  No tolerance is new.

Consecutive calls always get different frames (disjoint slices of one seeded draw).  No entry was found that is not
bit-reproducible by design: every sum of the library has a fixed order (include/vcmi.h).

Sizes: the long inputs are there because the state only changes at those sizes -- kSortMinFrames = 8192 (grouping),
nsuper = ceil(T / 1024 / 32) (super-chunk tables), nchunks > 1024 (group_super_shift 6), kMinChunkFrames = 98304 (staging
ring of the host entry), 65536 frames (hard-assignment E-step), kVcScratchKeepBytes = 256 MiB (release of the vc scratch).
No test here captures a call into a graph: DESIGN.md, "State that outlives a call", says why.
tests/test_call_history_host.py proves the geometry claims without a GPU."""
import functools
import sys

import numpy as np
import pytest

import call_history as ch
import mgc_restatement as mr
from conftest import frame_relerr, julia_model, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-9          # fvconvert, posteriors, E-step statistics
TRAJ_TOL = 1e-6     # behind the trajectory solve
MGC_TOL = 1e-12


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    m.set_devices([])
    return m


def dev(X):
    """(T,D) host rows -> the (D,T) device view the library takes"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(X)).cuda().t()


# ======================================================================================================================
# a. one GMMMap, many sizes
# ======================================================================================================================
@functools.lru_cache(maxsize=None)
def _peaked():
    import synthdata
    return synthdata.synth_model(1002, 80, 64, lam_lo=1e-5)


def _models(fixture_model):
    return {"peaked": _peaked(), "fixture": fixture_model}


def _gmm_call(vc, g, op, Xd):
    if op == "convert":
        return vc.fvconvert(g, Xd)
    if op == "predict":
        return vc.predict(g.px, Xd)
    return vc.predict_proba(g.px, Xd)


def _gmm_oracle(ref, op, X, got):
    """the head and the tail of a step against the oracle (all of it for a small step)"""
    for sl in ([slice(0, len(X))] if len(X) <= 256 else [slice(0, 128), slice(len(X) - 64, len(X))]):
        x = X[sl]
        if op == "convert":
            assert frame_relerr(got[:, sl], ref.fvconvert(x).T) < TOL
        elif op == "predict":
            assert np.array_equal(got[sl], ref.predict(x))
        else:
            assert np.max(np.abs(got[:, sl] - ref.predict_proba(x).T)) < TOL


def _run_gmm_sequence(vc, model, seq, seed):
    import synthdata
    from oracle import c_oracle as co
    w, mu, sig = model
    D = mu.shape[1] // 2
    steps = ch.sequence_frames(seq)
    X = synthdata.sample_frames(seed, w, mu, sig, steps[-1][3][1], 0, D)
    Xd = dev(X)
    g = vc.GMMMap(*julia_model(w, mu, sig))
    played = ch.play([(name, functools.partial(_gmm_call, vc, g, op, Xd[:, a:b])) for name, op, _, (a, b) in steps])
    ref = co.GMMMap(w, mu, sig)
    for name, op, T, (a, b) in steps:
        one = ch.fresh(lambda: ch.to_numpy(_gmm_call(vc, vc.GMMMap(*julia_model(w, mu, sig)), op, Xd[:, a:b])))
        assert ch.same_bits(played[name], one), f"step {name}: bits differ from the fresh call"
        _gmm_oracle(ref, op, X[a:b], played[name])
    return g


@pytest.mark.parametrize("which", ["peaked", "fixture"])
def test_fvconvert_many_sizes_on_one_handle(vc, fixture_model, which):
    """T = 8209, 100, 40 000, 8192, 70 001, 1, 8209, 40 000, 8191 on one handle: the super-chunk tables are allocated
    (nsuper 1), reallocated (2), reused by a smaller call (1), reallocated (3); calls under 8192 frames skip the grouping in
    between; call n adds into table n & 1 and clears the other for call n + 1."""
    g = _run_gmm_sequence(vc, _models(fixture_model)[which], [("convert", T) for T in ch.FVCONVERT_T], 4101)
    if which == "peaked":
        assert g.convert_plan()[1] == 3              # the screened shape: what the headline configuration runs


@pytest.mark.parametrize("which", ["peaked", "fixture"])
def test_convert_predict_posterior_interleaved_on_one_handle(vc, fixture_model, which):
    """the same sizes with predict and predict_proba in between (call_history.INTERLEAVED): the screened arg-max shares
    launch_grouping, its buffers and both tables with the convert kernels, in both orders"""
    _run_gmm_sequence(vc, _models(fixture_model)[which], ch.INTERLEAVED, 4102)


def test_prune_and_kernel_switches_and_an_argument_error_in_between(vc):
    """set_prune(inf) -> call -> set_prune(46) -> call, set_kernel(1) -> call -> set_kernel(0) -> call, and a refused call
    (DimensionMismatch) before the last one: the next call's bits are those of a fresh handle with the same setting"""
    import synthdata
    import torch
    from oracle import c_oracle as co
    w, mu, sig = _peaked()
    steps = ch.sequence_frames([("convert", T) for _, T in ch.TOGGLES] + [("convert", 8209)])
    X = synthdata.sample_frames(4103, w, mu, sig, steps[-1][3][1], 0, 40)
    Xd = dev(X)
    settings = [s for s, _ in ch.TOGGLES] + ["after_error"]

    def apply(g, setting):
        {"prune_inf": lambda: g.set_prune(float("inf")), "prune_46": lambda: g.set_prune(46.0),
         "kernel_1": lambda: g.set_kernel(1), "kernel_0": lambda: g.set_kernel(0), "after_error": lambda: None}[setting]()

    g = vc.GMMMap(*julia_model(w, mu, sig))
    ref = co.GMMMap(w, mu, sig)
    for setting, (name, _, _, (a, b)) in zip(settings, steps):
        if setting == "after_error":
            with pytest.raises(vc.DimensionMismatch):
                vc.fvconvert(g, torch.zeros((9000, 39), dtype=torch.float64, device="cuda").t())
            with pytest.raises(vc.DimensionMismatch):
                vc.fvconvert(g, np.zeros((41, 10)))
        apply(g, setting)
        got = ch.to_numpy(vc.fvconvert(g, Xd[:, a:b]))

        def one():
            h = vc.GMMMap(*julia_model(w, mu, sig))
            apply(h, setting)
            return ch.to_numpy(vc.fvconvert(h, Xd[:, a:b]))

        assert ch.same_bits(got, ch.fresh(one)), setting
        _gmm_oracle(ref, "convert", X[a:b], got)


def test_host_pointer_entry_many_sizes_ring_and_pinned_arrays(vc):
    """the same sizes through the host-pointer entry (numpy in and out), then 300 001 frames (several chunks through the
    staging ring), then 1 and 2000 frames (the utterance path that skips it); then the last three from a pin()-ed array
    (DMA straight from it) and again after unpin() (staged again).  Results are identical either way (include/vcmi.h)."""
    import synthdata
    from oracle import c_oracle as co
    w, mu, sig = _peaked()
    steps = ch.sequence_frames([("convert", T) for T in ch.HOST_T])
    X = synthdata.sample_frames(4104, w, mu, sig, steps[-1][3][1], 0, 40)
    Xj = np.asfortranarray(X.T)                       # (D, total): a column slice is one contiguous block of the image
    g = vc.GMMMap(*julia_model(w, mu, sig))
    played = ch.play([(name, functools.partial(vc.fvconvert, g, Xj[:, a:b])) for name, _, _, (a, b) in steps])
    ref = co.GMMMap(w, mu, sig)
    for name, _, _, (a, b) in steps:
        one = ch.fresh(lambda: vc.fvconvert(vc.GMMMap(*julia_model(w, mu, sig)), Xj[:, a:b]))
        assert ch.same_bits(played[name], one), name
        _gmm_oracle(ref, "convert", X[a:b], played[name])
    last3 = steps[-3:]
    vc.pin(Xj)
    try:
        assert vc.is_pinned(Xj)
        for name, _, _, (a, b) in last3:
            assert ch.same_bits(vc.fvconvert(g, Xj[:, a:b]), played[name]), f"pinned {name}"
    finally:
        vc.unpin(Xj)
    assert not vc.is_pinned(Xj)
    for name, _, _, (a, b) in last3:
        assert ch.same_bits(vc.fvconvert(g, Xj[:, a:b]), played[name]), f"after unpin {name}"


def test_more_than_1024_chunks_then_a_small_call_then_again(vc):
    """D = 16, M = 4, broad (lam_lo = 0.3): 1 050 000 frames are 1026 chunks -> group_super_shift 6 (17 super-chunks), 8193
    frames shift 5, then 1 050 000 other frames again.  The long ones: bit equality with the fresh call and < 1e-13 per frame
    against the same call without grouping (DBG_CONVERT_NO_GROUPING: frames in the caller's order); 8193: the oracle."""
    import synthdata
    from oracle import c_oracle as co
    from voiceconversion_jl_amd import _lib
    D, M = 16, 4
    w, mu, sig = synthdata.synth_model(1616, 2 * D, M, lam_lo=3e-1)
    steps = ch.sequence_frames([("convert", T) for T in ch.LONG_T])
    X = synthdata.sample_frames(4105, w, mu, sig, steps[-1][3][1], 0, D)
    Xd = dev(X)
    g = vc.GMMMap(*julia_model(w, mu, sig))
    played = ch.play([(name, functools.partial(vc.fvconvert, g, Xd[:, a:b])) for name, _, _, (a, b) in steps])
    for name, _, T, (a, b) in steps:
        one = ch.fresh(lambda: ch.to_numpy(vc.fvconvert(vc.GMMMap(*julia_model(w, mu, sig)), Xd[:, a:b])))
        assert ch.same_bits(played[name], one), name
        if T > 100_000:
            _lib.debug_force(_lib.DBG_CONVERT_NO_GROUPING)
            try:
                plain = ch.to_numpy(vc.fvconvert(g, Xd[:, a:b]))
            finally:
                _lib.debug_force(0)
            e = frame_relerr(played[name], plain)
            print(f"{name}: grouped against ungrouped {e:.2e}")
            assert e < 1e-13
        else:
            assert frame_relerr(played[name], co.GMMMap(w, mu, sig).fvconvert(X[a:b]).T) < TOL


# ======================================================================================================================
# b. two streams, no host synchronisation in between
# ======================================================================================================================
def _two_streams(callA, callB, rounds=3):
    """Reference results with a device synchronisation between the calls; then `rounds` times call A on s1 and call B on s2
    back to back (torch's streams are non-blocking), both outputs bit for bit.  The first round may still be serialised by
    the allocations of the streams' first outputs; the later ones are not."""
    import torch
    refA = ch.to_numpy(callA())
    torch.cuda.synchronize()
    refB = ch.to_numpy(callB())
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for r in range(rounds):
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            a = callA()
        with torch.cuda.stream(s2):
            b = callB()               # no host synchronisation in between
        torch.cuda.synchronize()
        assert ch.same_bits(ch.to_numpy(a), refA), f"round {r}: call A on stream 1"
        assert ch.same_bits(ch.to_numpy(b), refB), f"round {r}: call B on stream 2"
    return refA, refB


def _gmm_pair(vc, model, D, TA, TB, seed):
    import synthdata
    w, mu, sig = model
    X = synthdata.sample_frames(seed, w, mu, sig, TA + TB, 0, D)
    Xd = dev(X)
    return vc.GMMMap(*julia_model(w, mu, sig)), X, Xd[:, :TA], Xd[:, TA:]


def test_two_streams_convert_grouped(vc):
    """vcmi_gmmmap_convert_dev, D = 40, M = 64, grouped (grp_order): 300 000 and 200 001 frames, ~1.5 and ~1 ms"""
    from oracle import c_oracle as co
    g, X, A, B = _gmm_pair(vc, _peaked(), 40, 300_000, 200_001, 4201)
    ra, rb = _two_streams(lambda: vc.fvconvert(g, A), lambda: vc.fvconvert(g, B))
    ref = co.GMMMap(*_peaked())
    assert frame_relerr(ra[:, :256], ref.fvconvert(X[:256]).T) < TOL
    assert frame_relerr(rb[:, -256:], ref.fvconvert(X[-256:]).T) < TOL


@functools.lru_cache(maxsize=None)
def _model_d100():
    import synthdata
    return synthdata.synth_model(1100, 200, 8, lam_lo=1e-3)


@functools.lru_cache(maxsize=None)
def _model_d7():
    import synthdata
    return synthdata.synth_model(1107, 14, 6, lam_lo=1e-2)


def test_two_streams_convert_through_scratch_lp(vc):
    """vcmi_gmmmap_convert_dev at D = 100, M = 8: log-densities into the handle's scratch_lp, then the regression kernel reads
    them.  Without an order on scratch_lp the second call's log-densities overwrite the first call's while its regression
    kernel still reads them."""
    from oracle import c_oracle as co
    g, X, A, B = _gmm_pair(vc, _model_d100(), 100, 200_000, 150_001, 4202)
    ra, rb = _two_streams(lambda: vc.fvconvert(g, A), lambda: vc.fvconvert(g, B))
    ref = co.GMMMap(*_model_d100())
    assert frame_relerr(ra[:, :256], ref.fvconvert(X[:256]).T) < TOL
    assert frame_relerr(rb[:, -256:], ref.fvconvert(X[-256:]).T) < TOL


@pytest.mark.parametrize("D", [100, 7])
def test_two_streams_predict_two_pass(vc, D):
    """vcmi_gmmmap_predict_dev on the route without an in-kernel arg-max (D = 100: tiled log-densities; D = 7: the generic
    kernel): the (M,T) log-density matrix goes through scratch_lp"""
    from oracle import c_oracle as co
    model = _model_d100() if D == 100 else _model_d7()
    g, X, A, B = _gmm_pair(vc, model, D, 300_000, 200_001, 4203 + D)
    ra, rb = _two_streams(lambda: vc.predict(g.px, A), lambda: vc.predict(g.px, B))
    ref = co.GMMMap(*model)
    assert np.array_equal(ra[:512], ref.predict(X[:512])) and np.array_equal(rb[-512:], ref.predict(X[-512:]))


def test_two_streams_posterior(vc):
    """vcmi_gmmmap_posterior_dev writes the caller's buffer only: no shared scratch"""
    from oracle import c_oracle as co
    g, X, A, B = _gmm_pair(vc, _peaked(), 40, 300_000, 200_001, 4204)
    ra, rb = _two_streams(lambda: vc.predict_proba(g.px, A), lambda: vc.predict_proba(g.px, B))
    ref = co.GMMMap(*_peaked())
    assert np.max(np.abs(ra[:, :256] - ref.predict_proba(X[:256]).T)) < TOL
    assert np.max(np.abs(rb[:, -256:] - ref.predict_proba(X[-256:]).T)) < TOL


def _diag_case(seed, N, Dj, M, kind="apart"):
    """frames and a diagonal model: "apart" -- well-separated mixtures (every frame has an owner: the hard-assignment path
    from 65536 frames on); "overlap" -- means pulled together, broad variances (the path steps aside)"""
    import synthdata
    w, mu, _ = synthdata.synth_model(seed, Dj, M)
    rg = np.random.default_rng(seed + 1)
    if kind == "apart":
        mu = 4.0 * mu
        var = np.exp(rg.uniform(np.log(1e-2), 0.0, (M, Dj)))
    else:
        mu = 0.05 * mu
        var = np.exp(rg.uniform(np.log(0.5), np.log(2.0), (M, Dj)))
    comp = rg.choice(M, size=N, p=w)
    X = mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])
    return X, (w, np.asfortranarray(mu.T), np.asfortranarray(var.T)), (w, mu, var)


def _check_diag(vc, stats, X, ref_params):
    from oracle import c_oracle as co
    M, Dj = ref_params[1].shape
    S0, S1, S2, ll = vc.unpack_stats(stats, Dj, M)
    r0, r1, r2, rl = co.estep_diag(X, *ref_params)
    assert relerr(S0, r0) < TOL and relerr(S1, r1.T) < TOL and relerr(S2, r2.T) < TOL and abs(ll - rl) < TOL * abs(rl)


def _full_case(seed, N, Dj, M):
    import synthdata
    w, mu, sig = synthdata.synth_model(seed, Dj, M, lam_lo=1e-2)
    X = synthdata.sample_frames(seed + 1, w, mu, sig, N, 0, Dj)
    return X, julia_model(w, mu, sig), (w, mu, sig)


def _check_full(vc, stats, X, ref_params):
    from oracle import c_oracle as co
    M, Dj = ref_params[1].shape
    S0, S1, S2, ll = vc.unpack_full_stats(stats, Dj, M)
    r0, r1, r2, rl = co.estep_full(X, *ref_params)
    assert relerr(S0, r0) < TOL and relerr(S1, r1.T) < TOL and relerr(S2, np.transpose(r2, (2, 1, 0))) < TOL
    assert abs(ll - rl) < TOL * abs(rl)


def test_two_streams_estep_diag(vc):
    """vcmi_estep_diag_dev: the hard-assignment path (70 000 x 80 x 128) on one stream, the one-tile kernel (40 000 x 80 x 16)
    on the other; both use the thread's EstepScratch and its parameter staging ring under one StreamOrder"""
    XA, pA, _ = _diag_case(4210, 70_000, 80, 128)
    XB, pB, rB = _diag_case(4211, 40_000, 80, 16)
    A, B = dev(XA), dev(XB)
    ra, rb = _two_streams(lambda: vc.estep_diag_dev(A, *pA), lambda: vc.estep_diag_dev(B, *pB))
    assert abs(ra[:128].sum() - 70_000) < 1e-6 * 70_000
    _check_diag(vc, rb, XB, rB)


def test_two_streams_estep_full(vc):
    """vcmi_estep_full_dev, 20 000 x 80 x 64 and 5000 x 160 x 6 (the thread's p(x) handle is prepared in place for each)"""
    XA, pA, _ = _full_case(4220, 20_000, 80, 64)
    XB, pB, rB = _full_case(4222, 5000, 160, 6)
    A, B = dev(XA), dev(XB)
    ra, rb = _two_streams(lambda: vc.estep_full_dev(A, *pA), lambda: vc.estep_full_dev(B, *pB))
    assert abs(ra[:64].sum() - 20_000) < 1e-6 * 20_000
    _check_full(vc, rb, XB, rB)


def _check_mc2sp(sp, mc, alpha, fftlen):
    lr = np.log(mr.mc2sp(mc, alpha, fftlen))
    err = np.max(np.abs(np.log(sp) - lr), axis=0)
    tol = MGC_TOL * np.maximum(1.0, np.max(np.abs(lr), axis=0))
    print(f"mc2sp D={mc.shape[0]} alpha={alpha} fftlen={fftlen}: max log error {err.max():.2e} (bar {tol.min():.1e})")
    assert np.all(err <= tol)


def _check_sp2mc(mc, sp, order, alpha):
    ref = mr.sp2mc(sp, order, alpha)
    err = np.max(np.abs(mc - ref), axis=0)
    tol = MGC_TOL * np.maximum(1.0, np.max(np.abs(np.log(sp)), axis=0))
    print(f"sp2mc K={sp.shape[0]} order={order} alpha={alpha}: max error {err.max():.2e} (bar {tol.min():.1e})")
    assert np.all(err <= tol)


def test_two_streams_mc2sp_and_sp2mc(vc):
    """vcmi_mc2sp_dev / vcmi_sp2mc_dev with two (D, alpha, fftlen) in turn: each call rebuilds the thread's one cached folded
    matrix (behind a device-wide wait) while the other stream's kernel may still be reading the old one"""
    T = 20_000
    (DA, aA, fA), (DB, aB, fB) = ch.MGC_A, ch.MGC_B
    mcA, mcB = mr.smooth_mc(4230, DA, T, c0=-2.0), mr.smooth_mc(4231, DB, T, c0=-2.0)
    A, B = dev(mcA.T), dev(mcB.T)
    ra, rb = _two_streams(lambda: vc.mc2sp(A, aA, fA), lambda: vc.mc2sp(B, aB, fB))
    _check_mc2sp(ra[:, :64], mcA[:, :64], aA, fA)
    _check_mc2sp(rb[:, -64:], mcB[:, -64:], aB, fB)
    spA, spB = dev(np.ascontiguousarray(ra.T)), dev(np.ascontiguousarray(rb.T))
    sa, sb = _two_streams(lambda: vc.sp2mc(spA, DA - 1, aA), lambda: vc.sp2mc(spB, DB - 1, aB))
    _check_sp2mc(sa[:, :64], ra[:, :64], DA - 1, aA)
    _check_sp2mc(sb[:, -64:], rb[:, -64:], DB - 1, aB)


def test_two_streams_variance_scaling_and_push_delta(vc):
    """vcmi_variance_scaling_dev with two sigma2 vectors (the thread's statistics scratch, its own StreamOrder) and
    vcmi_push_delta_dev (no scratch at all)"""
    from oracle import c_oracle as co
    rng = np.random.default_rng(4240)
    XA, XB = rng.standard_normal((300_000, 40)) * 2.0 + 1.0, rng.standard_normal((200_001, 25)) * 0.5 - 1.0
    vsA, vsB = vc.VarianceScaling(rng.uniform(0.5, 2.0, 40)), vc.VarianceScaling(rng.uniform(0.5, 2.0, 25))
    A, B = dev(XA), dev(XB)
    ra, rb = _two_streams(lambda: vc.fvpostf(vsA, A), lambda: vc.fvpostf(vsB, B))
    assert relerr(ra, co.variance_scaling(XA, vsA.sigma2).T) < 1e-12            # (the bar of test_gpu_postf.py)
    assert relerr(rb, co.variance_scaling(XB, vsB.sigma2).T) < 1e-12
    pa, pb = _two_streams(lambda: vc.push_delta(A), lambda: vc.push_delta(B))
    assert np.array_equal(pa, co.push_delta(XA).T) and np.array_equal(pb, co.push_delta(XB).T)


@functools.lru_cache(maxsize=None)
def _traj_model(Ds=12, M=4, seed=311):
    import synthdata
    return synthdata.synth_model(seed, 4 * Ds, M, lam_lo=1e-3)


def _static(seed, model, T, Ds):
    import synthdata
    w, mu, sig = model
    st = synthdata.sample_frames(seed, w, mu, sig, T, 0, Ds)
    return np.cumsum(st, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]


def _gv_stats(Ds):
    rng = np.random.default_rng(77)
    muv = rng.uniform(0.5, 1.5, Ds)
    A = rng.standard_normal((Ds, Ds))
    return muv, A @ A.T / Ds * np.mean(muv) ** 2 * 0.1 + np.diag(muv ** 2 * 0.05)


def test_two_streams_trajectory_entries(vc):
    """vcmi_vc_traj_dev, vcmi_traj_convert_batch_dev and vcmi_vc_trajgv_dev / vcmi_trajgv_convert_batch_dev, each pair on ONE
    converter.  These entries end with the read of the solver's status word, which waits for their stream: a call has finished
    when it returns, so two of them cannot overlap whatever streams they use -- the test holds that."""
    import torch
    from oracle import c_oracle as co
    from voiceconversion_jl_amd import _lib
    Ds, L = 12, 100
    model = _traj_model()
    g = vc.GMMMap(*julia_model(*model))
    tj = vc.TrajectoryGMMMap(g, L)
    muv, Sv = _gv_stats(Ds)
    tgv = vc.TrajectoryGVGMMMap(vc.TrajectoryGMMMap(g, L), muv, Sv)
    stA, stB = _static(4250, model, 20_000, Ds), _static(4251, model, 12_000, Ds)
    fmA = np.hstack([np.linspace(0, 1, len(stA))[:, None], stA])
    fmB = np.hstack([np.linspace(1, 2, len(stB))[:, None], stB])
    A, B = dev(fmA), dev(fmB)
    ref = co.TrajectoryGMMMap(co.GMMMap(*model))

    # the chunk length is state too: vc leaves length(c) at the last chunk's length, which is the NEXT call's chunk length
    # (src/common.jl:41).  One converter serves both streams here, so both matrices are whole chunks of L.
    A, B = A[:, :20_000], B[:, :12_000]
    ra, rb = _two_streams(lambda: vc.vc(tj, A, delta=True), lambda: vc.vc(tj, B, delta=True))
    want = ref.vc(np.hstack([fmA[:300, :1], co.push_delta(stA)[:300]]), L)
    assert relerr(ra[1:, :200], want[:200, 1:].T) < TRAJ_TOL and np.array_equal(ra[0], fmA[:20_000, 0])
    ga, gb = _two_streams(lambda: tgv._vc(A[:, :3000], delta=True, epochs=20), lambda: tgv._vc(B[:, :2000], delta=True, epochs=20))
    assert np.all(np.isfinite(ga)) and np.all(np.isfinite(gb))

    # the raw batch entries: utterances of L frames at offsets into one device buffer
    def batch(entry_args, Xd, n):
        D2 = 2 * Ds
        T = np.full(n, L, dtype=np.int64)
        xo, yo = np.arange(n, dtype=np.int64) * L * D2, np.arange(n, dtype=np.int64) * L * Ds
        Y = torch.empty((n * L, Ds), dtype=torch.float64, device="cuda")
        _lib.check(entry_args(n, Xd.data_ptr(), _lib.iptr(xo), _lib.iptr(T), Y.data_ptr(), _lib.iptr(yo),
                              torch.cuda.current_stream().cuda_stream))
        return Y

    XA, XB = vc.push_delta(A[1:]).t().contiguous(), vc.push_delta(B[1:]).t().contiguous()     # (T, 2Ds) dense
    torch.cuda.synchronize()

    def traj_entry(n, x, xo, T, y, yo, s):
        return _lib.lib.vcmi_traj_convert_batch_dev(tj._h, n, x, xo, T, y, yo, s)

    def gv_entry(n, x, xo, T, y, yo, s):
        return _lib.lib.vcmi_trajgv_convert_batch_dev(tgv._h, n, x, xo, T, 20, 1.0e-5, y, yo, s)

    ba, bb = _two_streams(lambda: batch(traj_entry, XA, 200), lambda: batch(traj_entry, XB, 120))
    y0, _, _ = ref.fvconvert(XA[:L].cpu().numpy())
    assert relerr(ba[:L], y0) < TRAJ_TOL
    _two_streams(lambda: batch(gv_entry, XA, 30), lambda: batch(gv_entry, XB, 20))


def test_two_streams_em_handles(vc):
    """vcmi_gmm_em_estep_dev and vcmi_gmm_em_diag_estep_dev, two frame blocks on ONE handle each: the handle's parameters are
    read only, the statistics go through the thread's E-step scratch (StreamOrder)"""
    X, pA, rA = _full_case(4260, 29_000, 48, 8)
    XA, XB = X[:20_000], X[20_000:]
    em = vc.EMState(*pA)
    A, B = dev(XA), dev(XB)
    ra, rb = _two_streams(lambda: em.estep(A), lambda: em.estep(B))
    _check_full(vc, rb, XB, rA)
    X, pC, rC = _diag_case(4264, 35_000, 80, 16)
    XC, XD = X[:30_000], X[30_000:]
    emd = vc.DiagEMState(*pC)
    Cd, Dd = dev(XC), dev(XD)
    rc, rd = _two_streams(lambda: emd.estep(Cd), lambda: emd.estep(Dd))
    _check_diag(vc, rd, XD, rC)
    assert ch.same_bits(rc, ch.to_numpy(vc.estep_diag_dev(Cd, *pC)))            # (include/vcmi.h: bit-identical)


def test_two_streams_kmeans_assign_needs_the_caller_s_order(vc):
    """vcmi_kmeans_assign_dev keeps labels, mind2 and the statistics partials on the HANDLE with no order of its own:
    include/vcmi.h asks the caller to order two calls of one handle on different streams.  With that order (the second stream
    waits for the first) the results are those of synchronised calls."""
    import torch
    km = sys.modules["voiceconversion_jl_amd.kmeans"]
    rng = np.random.default_rng(4270)
    Dj, M = 24, 64
    XA, XB = rng.standard_normal((300_000, Dj)) + 2.0, rng.standard_normal((200_001, Dj)) - 1.0
    C = XA[rng.choice(len(XA), M, replace=False)]
    st = km.KMeansState(Dj, M, C.T)
    A, B = dev(XA), dev(XB)
    refA = ch.to_numpy(st.assign(A))
    torch.cuda.synchronize()
    refB = ch.to_numpy(st.assign(B))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for r in range(3):
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            a = st.assign(A)
        s2.wait_stream(s1)                        # the caller's order, no host synchronisation
        with torch.cuda.stream(s2):
            b = st.assign(B)
        torch.cuda.synchronize()
        assert ch.same_bits(ch.to_numpy(a), refA) and ch.same_bits(ch.to_numpy(b), refB), r
    assert refA[:M].sum() == len(XA) and refB[:M].sum() == len(XB)
    # ... and a small block afterwards, on the same handle, against the restatement
    import kmeans_restatement as kr
    small = ch.to_numpy(st.assign(dev(XB[:3001])))
    lab, d2 = kr.assign(XB[:3001], C)
    assert np.array_equal(small[:M], np.bincount(lab, minlength=M).astype(float)) and abs(small[-1] - d2.sum()) <= 1e-12 * d2.sum()


# ======================================================================================================================
# c. a failing call, then a good one
# ======================================================================================================================
def _half_bad_model(Ds, seed):
    """M = 2 over (static, delta) source and target features: mixture 0 an ordinary SPD joint covariance, mixture 1 the
    [[I, 2I], [2I, I]] block of test_not_positive_definite_normal_matrix (p(x) is fine, the conditional covariance is negative
    definite).  Static source means 50 apart, delta means 0: an utterance near mean 0 converts with mixture 0 alone, one near
    mean 1 selects mixture 1 and the solve reports W'D^-1W not positive definite."""
    import synthdata
    w0, mu0, sig0 = synthdata.synth_model(seed, 4 * Ds, 1, lam_lo=1e-3)
    I = np.eye(2 * Ds)
    sig = np.stack([sig0[0], np.block([[I, 2.0 * I], [2.0 * I, I]])])
    mu = np.stack([mu0[0], np.random.default_rng(seed + 1).standard_normal(4 * Ds)])
    mu[0, :2 * Ds] = 0.0
    mu[1, :Ds] = 50.0
    mu[1, Ds:2 * Ds] = 0.0
    good = (np.ones(1), mu[:1].copy(), sig[:1].copy())           # what a good utterance's conversion is, for the oracle
    return (np.array([0.5, 0.5]), mu, sig), good


def _utterance(seed, good_model, T, Ds, shift=0.0):
    from oracle import c_oracle as co
    return np.asfortranarray(co.push_delta(_static(seed, good_model, T, Ds) + shift).T)      # (2Ds, T)


@pytest.mark.parametrize("solver,Ds", [("blocked", 12), ("generic", 12), ("big", 50)])
def test_trajectory_good_bad_good(vc, solver, Ds):
    """good, bad (PosDefException), good, the batch [good, bad, good] (raises), good again -- on one converter, for the
    MFMA-blocked solver, the runtime-D kernel (DBG_TRAJ_GENERIC) and the big-D kernel (D = 50): the status word a failing
    solve wrote is cleared by the next call's hipMemsetAsync, and nothing else of the failed call stays behind.
    With this model vcmi_traj_set_em(t, 2) is itself a failing call (VCMI_ERR_NOT_PD: the EM objective needs every
    (Q_m + Q_m')/2 positive definite, include/vcmi.h), so what is held for EM is that the refusal leaves em_iters at 0 and
    the next conversion's bits alone; test_gv_refuses_em_then_converts covers the GV converter's refusal on a good model."""
    from oracle import c_oracle as co
    from voiceconversion_jl_amd import _lib
    model, good_model = _half_bad_model(Ds, 900 + Ds)
    T = 60
    g1, g2 = _utterance(4301, good_model, T, Ds), _utterance(4302, good_model, 41, Ds)
    bad = _utterance(4303, good_model, 33, Ds)
    bad[:Ds] += 50.0
    flags = _lib.DBG_TRAJ_GENERIC if solver == "generic" else 0

    def forced(fn):
        _lib.debug_force(flags)
        try:
            return fn()
        finally:
            _lib.debug_force(0)

    def make():
        return vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*model)), T)

    t = make()
    fresh1 = ch.fresh(lambda: forced(lambda: vc.fvconvert(make(), g1)))
    fresh2 = ch.fresh(lambda: forced(lambda: vc.fvconvert(make(), g2)))
    ref = co.TrajectoryGMMMap(co.GMMMap(*good_model))
    assert relerr(fresh1, ref.fvconvert(g1.T)[0].T) < TRAJ_TOL and relerr(fresh2, ref.fvconvert(g2.T)[0].T) < TRAJ_TOL

    def step():
        assert ch.same_bits(forced(lambda: vc.fvconvert(t, g1)), fresh1)
        with pytest.raises(vc.PosDefException):
            forced(lambda: vc.fvconvert(t, bad))
        assert ch.same_bits(forced(lambda: vc.fvconvert(t, g2)), fresh2), "the good call after the failing one"
        with pytest.raises(vc.PosDefException):
            forced(lambda: t.fvconvert_batch([g1, bad, g2]))
        assert ch.same_bits(forced(lambda: vc.fvconvert(t, g1)), fresh1), "the good call after the failing batch"
        both = forced(lambda: t.fvconvert_batch([g2, g1]))
        assert ch.same_bits(both[0], fresh2) and ch.same_bits(both[1], fresh1)

    step()
    with pytest.raises(vc.PosDefException):
        t.em_iters = 2
    assert t.em_iters == 0
    step()


def test_gv_refuses_em_then_converts(vc):
    """a GV converter over a trajectory handle with em_iters > 0 returns VCMI_ERR_ARG before anything runs; with em_iters back
    at 0 it converts to the bits it gave before and to those of a fresh pair of handles"""
    Ds, T = 12, 50
    model = _traj_model()
    X1, X2 = _utterance(4311, model, T, Ds), _utterance(4312, model, 37, Ds)
    muv, Sv = _gv_stats(Ds)

    def make():
        t = vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*model)), T)
        return t, vc.TrajectoryGVGMMMap(t, muv, Sv)

    t, tgv = make()
    before = vc.fvconvert(tgv, X1, epochs=20)
    t.em_iters = 2
    with pytest.raises(vc.VCMIError):
        vc.fvconvert(tgv, X2, epochs=20)
    plain_em = vc.fvconvert(t, X2)                           # the plain converter runs EM meanwhile (its scratch on the handle)
    assert np.all(np.isfinite(plain_em))
    t.em_iters = 0
    assert ch.same_bits(vc.fvconvert(tgv, X1, epochs=20), before)
    assert ch.same_bits(before, ch.fresh(lambda: vc.fvconvert(make()[1], X1, epochs=20)))
    assert ch.same_bits(vc.fvconvert(tgv, X2, epochs=20), ch.fresh(lambda: vc.fvconvert(make()[1], X2, epochs=20)))


def test_sp2mc_refused_spectrum_then_a_good_one(vc):
    """the host entry raises for a non-positive power (the kernel sets the thread's flag word); the next call on the thread
    starts from a cleared flag and gives the fresh bits"""
    K, order, alpha, T = 513, 40, 0.41, 300
    sp1, sp2 = (np.exp(np.random.default_rng(s).standard_normal((K, T))) for s in (4321, 4322))
    bad = sp2.copy()
    bad[100, 17] = -1.0
    first = vc.sp2mc(sp1, order, alpha)
    with pytest.raises(vc.VCMIError):
        vc.sp2mc(bad, order, alpha)
    second = vc.sp2mc(sp2, order, alpha)
    assert ch.same_bits(second, ch.fresh(lambda: vc.sp2mc(sp2, order, alpha)))
    assert ch.same_bits(vc.sp2mc(sp1, order, alpha), first)
    _check_sp2mc(second, sp2, order, alpha)


def test_kmeans_nan_frame_then_a_clean_block_on_the_same_handle(vc):
    """test_errors of test_gpu_kmeans.py runs a whole new kmeans() after a refused one (a new handle).  Missing there: the SAME
    handle -- an assignment over a block with a NaN frame raises the handle's flag, vcmi_kmeans_update reports it
    (VCMI_ERR_ARG, kmeans.hip km_read_flag) and clears it; with the centers set again, the next assignment and update are
    those of a fresh handle."""
    import kmeans_restatement as kr
    km = sys.modules["voiceconversion_jl_amd.kmeans"]
    rng = np.random.default_rng(4330)
    Dj, M, N = 24, 9, 5000
    X1, X2 = rng.standard_normal((N, Dj)) + 2.0, rng.standard_normal((N + 3, Dj)) + 2.0
    C = X1[rng.choice(N, M, replace=False)].copy()
    Xn = X1.copy()
    Xn[1234, 5] = np.nan

    def clean(st):
        stats = st.assign(dev(X2))
        return ch.to_numpy(stats), st.update(stats), st.get()

    st = km.KMeansState(Dj, M, C.T)
    with pytest.raises(vc.VCMIError):
        st.update(st.assign(dev(Xn)))
    st.set(C.T)
    got = clean(st)
    want = ch.fresh(lambda: clean(km.KMeansState(Dj, M, C.T)))
    assert ch.same_bits(got[0], want[0]) and got[1] == want[1] and ch.same_bits(got[2], want[2])
    lab, d2 = kr.assign(X2, C)
    assert np.array_equal(got[0][:M], np.bincount(lab, minlength=M).astype(float))
    assert abs(got[0][-1] - d2.sum()) <= 1e-12 * d2.sum()


def test_estep_full_bad_model_then_the_good_one(vc):
    """estep_full with mixture 3 of 4 negated (VCMI_ERR_NOT_PD from the device Cholesky's flag), then the good model: the
    thread's p(x) handle, parameter staging and flag are rewritten"""
    X, p, r = _full_case(4340, 3000, 48, 4)
    X2 = _full_case(4342, 2500, 48, 4)[0]
    w, mu, sig = p
    neg = sig.copy()
    neg[:, :, 2] = -neg[:, :, 2]
    A, B = dev(X), dev(X2)
    first = ch.to_numpy(vc.estep_full_dev(A, w, mu, sig))
    with pytest.raises(vc.PosDefException, match="3"):
        vc.estep_full_dev(B, w, mu, neg)
    second = ch.to_numpy(vc.estep_full_dev(B, w, mu, sig))
    assert ch.same_bits(second, ch.fresh(lambda: ch.to_numpy(vc.estep_full_dev(B, w, mu, sig))))
    assert ch.same_bits(ch.to_numpy(vc.estep_full_dev(A, w, mu, sig)), first)
    _check_full(vc, second, X2, r)
    with pytest.raises(vc.PosDefException):
        vc.estep_full(X2.T, w, mu, neg)                        # the host entry
    S = vc.estep_full(X2.T, w, mu, sig)
    assert ch.same_bits(ch.to_numpy(S[:3]), ch.to_numpy(ch.fresh(lambda: vc.estep_full(X2.T, w, mu, sig))[:3]))


def test_gmmmap_construction_fails_then_succeeds_on_the_same_thread(vc):
    import synthdata
    from oracle import c_oracle as co
    w, mu, sig = synthdata.synth_model(4350, 48, 6)
    X = synthdata.sample_frames(4351, w, mu, sig, 9000, 0, 24)
    bad = sig.copy()
    bad[4, :24, :24] = -bad[4, :24, :24]

    def run():
        with pytest.raises(vc.PosDefException):
            vc.GMMMap(*julia_model(w, mu, bad))
        return ch.to_numpy(vc.fvconvert(vc.GMMMap(*julia_model(w, mu, sig)), dev(X)))

    got = run()
    assert ch.same_bits(got, ch.fresh(lambda: ch.to_numpy(vc.fvconvert(vc.GMMMap(*julia_model(w, mu, sig)), dev(X)))))
    assert ch.same_bits(got, ch.fresh(run))
    assert frame_relerr(got[:, :256], co.GMMMap(w, mu, sig).fvconvert(X[:256]).T) < TOL


# ======================================================================================================================
# d. thread-local scratch across shapes
# ======================================================================================================================
def test_estep_diag_scratch_across_shapes(vc):
    """(70 000, 80, 128) on the hard-assignment path -> (31, 80, 128) -> (4000, 80, 16) one-tile kernel -> (3000, 48, 128) ->
    (2000, 79, 20) odd dimension -> (70 000, 80, 128) with other frames and overlapping mixtures (the path steps aside)"""
    from voiceconversion_jl_amd import _lib
    cases = [(f"{i}_{N}x{Dj}x{M}_{kind}", _diag_case(4400 + 2 * i, N, Dj, M, kind)) for i, (N, Dj, M, kind) in enumerate(ch.ESTEP_DIAG_SHAPES)]
    devs = {name: dev(X) for name, (X, _, _) in cases}
    soft = {}

    def call(name, p):
        out = vc.estep_diag_dev(devs[name], *p)
        soft[name] = _lib.estep_last_soft()
        return out

    played = ch.play([(name, functools.partial(call, name, p)) for name, (_, p, _) in cases])
    first, last = cases[0][0], cases[-1][0]
    print(f"frames through the FP64 kernel after the screen: {soft[first]} of 70000 (apart), {soft[last]} (overlap)")
    assert 0 <= soft[first] < 70_000 // 4 and (soft[last] == -1 or soft[last] >= 3 * 70_000 // 4)
    for name, (X, p, r) in cases:
        assert ch.same_bits(played[name], ch.fresh(lambda: ch.to_numpy(vc.estep_diag_dev(devs[name], *p)))), name
        if len(X) <= 4000:
            _check_diag(vc, played[name], X, r)
        else:
            assert abs(played[name][:128].sum() - len(X)) < 1e-6 * len(X)


def test_estep_full_scratch_across_shapes(vc):
    """(20 000, 80, 64) -> (1, 80, 3) -> (5000, 160, 6) -> (1500, 48, 8): one thread-local p(x) handle re-prepared in place"""
    cases = [(f"{i}_{N}x{Dj}x{M}", _full_case(4420 + 2 * i, N, Dj, M)) for i, (N, Dj, M) in enumerate(ch.ESTEP_FULL_SHAPES)]
    devs = {name: dev(X) for name, (X, _, _) in cases}
    played = ch.play([(name, functools.partial(vc.estep_full_dev, devs[name], *p)) for name, (_, p, _) in cases])
    for name, (X, p, r) in cases:
        assert ch.same_bits(played[name], ch.fresh(lambda: ch.to_numpy(vc.estep_full_dev(devs[name], *p)))), name
        if len(X) <= 5000:
            _check_full(vc, played[name], X, r)


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_mgc_matrix_cache_across_shapes_and_alpha(vc, entry):
    """mc2sp / sp2mc / mc2b with shape A (D = 41, alpha = 0.41, fftlen 1024), B (25, 0.58, 512), A, C (A with alpha = 0.42), A:
    the thread caches ONE folded matrix per direction, keyed by (D, fftlen, alpha) / (K, order, alpha), and rebuilds it inside a
    grow-only buffer.  Every step against the fresh thread's bits and the restatement; A and C differ by far more than the bar."""
    T = 300
    data = {}
    for i, (name, (D, alpha, fftlen)) in enumerate(ch.MGC_SHAPES):
        data[name] = (mr.smooth_mc(4440 + i, D, T, c0=-2.0), D, alpha, fftlen)       # other frames at every step

    def arg(a):
        return dev(a.T) if entry == "dev" else a

    def call(name):
        mc, D, alpha, fftlen = data[name]
        sp = vc.mc2sp(arg(mc), alpha, fftlen)
        sp_host = ch.to_numpy(sp)
        back = vc.sp2mc(arg(sp_host), D - 1, alpha)
        return sp_host, ch.to_numpy(back), ch.to_numpy(vc.mc2b(arg(mc), alpha))

    played = ch.play([(name, functools.partial(call, name)) for name, _ in ch.MGC_SHAPES])
    for name, _ in ch.MGC_SHAPES:
        mc, D, alpha, fftlen = data[name]
        sp, back, b = played[name]
        assert ch.same_bits(played[name], ch.fresh(lambda: call(name))), f"mgc step {name}: bits differ from the fresh call"
        _check_mc2sp(sp, mc, alpha, fftlen)
        _check_sp2mc(back, sp, D - 1, alpha)
        rb = mr.mc2b(mc, alpha)
        assert np.max(np.abs(b - rb)) <= 1e-13 * np.max(np.abs(rb))
    mcC, D, alphaC, fftlen = data["C"]
    assert np.max(np.abs(np.log(played["C"][0]) - np.log(mr.mc2sp(mcC, ch.MGC_A[1], fftlen)))) > 1e-6     # alpha matters


def _warped_pair(rng, S, T, D):
    t = rng.standard_normal((S, D))
    idx = np.clip(np.sort(rng.integers(0, S, T)), 0, S - 1)
    return t, t[idx] + 0.2 * rng.standard_normal((T, D))


def test_dtw_scratch_across_shapes(vc):
    """200 pairs of the batch of test_fused_kernel_more_workgroups_than_slots (two-strip pairs included) -> one (3, 9, 47)
    pair -> (7000, 600) on the HBM scratch -> the small pair -> (60, 12 000), the two-kernel fallback -> align_batch of five
    pairs: every path exact against the oracle, so a step needs no fresh twin"""
    from oracle import c_oracle as co
    rng = np.random.default_rng(77)
    many = [_warped_pair(rng, int(rng.integers(20, 140)), int(rng.integers(20, 90)), 16) for _ in range(180)]
    many += [_warped_pair(rng, int(rng.integers(513, 700)), int(rng.integers(20, 60)), 16) for _ in range(20)]
    small = _warped_pair(rng, 3, 9, 47)
    small2 = _warped_pair(rng, 3, 9, 47)
    long_t = _warped_pair(rng, 7000, 600, 6)
    long_s = _warped_pair(rng, 60, 12_000, 8)
    five = [_warped_pair(rng, int(rng.integers(30, 600)), int(rng.integers(30, 300)), 16) for _ in range(5)]
    d = vc.DTW(fstep=0, bstep=2)

    def paths(pairs):
        return vc.fit_batch(d, [t.T for t, _ in pairs], [s.T for _, s in pairs])

    def exact(pairs, got, idx=None):
        for i in (idx if idx is not None else range(len(pairs))):
            assert np.array_equal(got[i], co.dtw_fit(pairs[i][0], pairs[i][1], 0, 2, tables=False)), i

    exact(many, paths(many), list(range(0, 200, 9)) + list(range(180, 200)))
    exact([small], paths([small]))
    exact([long_t], paths([long_t]))
    exact([small2], paths([small2]))
    exact([long_s], paths([long_s]))
    outs = vc.align_batch([t.T for t, _ in five], [s.T for _, s in five])
    for (t, s), o in zip(five, outs):
        assert np.array_equal(o[1], co.align(t, s)[0].T)
    exact(many[:40], paths(many[:40]))


def test_parallel_dataset_scratch_across_sizes(vc):
    """three pairs -> one shorter pair -> the three again (other data each time): the thread's DatasetScratch grows, is reused
    by a smaller call, and is reused at its size; each matrix equals the oracle's bit for bit"""
    import dataset_cases as dc
    from oracle import c_oracle as co
    rng = np.random.default_rng(4460)

    def pairs(shapes):
        out = []
        for S, T in shapes:
            src = dc.mcep(rng, S, 25)
            out.append((src, dc.warped_copy(rng, src, T)))
        return out

    for shapes in ([(120, 130), (257, 300), (90, 80)], [(33, 40)], [(120, 130), (257, 300), (90, 80)]):
        ps = pairs(shapes)
        ds = vc.ParallelDataset([(s.T, t.T) for s, t in ps], alpha=0.41, fftlen=256)
        want = np.concatenate([co.joint_features(*co.align_mcep(s, t, 0.41, 256), True, False, False) for s, t in ps], axis=0)
        assert len(ds) == want.shape[0] and np.array_equal(ds.X.t().cpu().numpy(), want)


def test_postf_and_push_delta_scratch_across_shapes(vc):
    """fvpostf / push_delta at D = 40 with 300 001 frames -> D = 7 with 3 -> D = 256 with 50, host and device entries"""
    from oracle import c_oracle as co
    rng = np.random.default_rng(4470)
    cases = {f"{D}x{T}": (rng.standard_normal((T, D)) * rng.uniform(0.1, 3.0, D) + rng.standard_normal(D),
                          vc.VarianceScaling(rng.uniform(0.5, 2.0, D))) for D, T in ch.POSTF_SHAPES}

    def call(name):
        X, vs = cases[name]
        Xj = np.asfortranarray(X.T)
        return (vc.fvpostf(vs, Xj), ch.to_numpy(vc.fvpostf(vs, dev(X))), vc.push_delta(Xj), ch.to_numpy(vc.push_delta(dev(X))))

    played = ch.play([(name, functools.partial(call, name)) for name in cases])
    for name, (X, vs) in cases.items():
        host, devr, pd, pdd = played[name]
        assert ch.same_bits(played[name], ch.fresh(lambda: call(name))), name
        assert np.array_equal(host, devr) and np.array_equal(pd, pdd) and np.array_equal(pd, co.push_delta(X).T)
        assert relerr(host, co.variance_scaling(X, vs.sigma2).T) < 1e-12


# ======================================================================================================================
# e. the 256 MiB release rule
# ======================================================================================================================
def test_vc_scratch_grow_release_grow(vc):
    """VcScratch::bytes() = 8 (x.n + y.n + stage.n); a host-pointer vc entry frees the three buffers on return above
    kVcScratchKeepBytes = 256 MiB.  vc(t, fm, postfilter) of a D = 12 trajectory converter (vcmi_vc_traj_postf; without the
    filter vc(t, fm) is the host-batch path, which has no such scratch) holds (2D,T) + (D,T) + the (2D+1,T) staging matrix with
    the (D+1,T) result behind it = (6D+2) T doubles: 460 000 frames are 272 MB.  vc(g, fm, postfilter) of a D = 40 GMMMap holds
    2 (D+1) T doubles in the staging matrix: 420 000 frames are 275 MB.  Before and after each long call a 300-frame call of the
    same kind: its bits must not move.  Chunks of L = 100 frames are independent: the first 300 columns of the long UNFILTERED
    result are the 300-frame call's (the filter's statistics are over the whole matrix, so the filtered long result is held to
    the library's two separate calls instead, at the 1e-13 of test_gpu_postf.py).
    The test cannot see whether the release happened: it covers the sequence grow -> (release) -> grow."""
    import synthdata
    from oracle import c_oracle as co
    Ds, L = 12, 100
    model = _traj_model()
    Tl = 460_000
    assert (6 * Ds + 2) * Tl * 8 > 256 << 20
    st = _static(4501, model, 4000, Ds)
    st = np.tile(st, (Tl // 4000, 1)) + 1e-3 * np.arange(Tl)[:, None] / Tl            # long, cheap to draw, no two chunks alike
    X = np.asfortranarray(np.vstack([np.linspace(0, 1, Tl)[None], vc.push_delta(np.asfortranarray(st.T))]))     # (2Ds+1, Tl)
    vs = vc.VarianceScaling(np.random.default_rng(2).uniform(0.5, 2.0, Ds))

    def make():
        return vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*model)), L)

    tj = make()
    small_plain, small = vc.vc(tj, X[:, :300]), vc.vc(tj, X[:, :300], postfilter=vs)
    ref = co.TrajectoryGMMMap(co.GMMMap(*model)).vc(np.ascontiguousarray(X[:, :300].T), L)
    assert relerr(small_plain, ref.T) < TRAJ_TOL
    assert relerr(small[1:], co.variance_scaling(np.ascontiguousarray(ref[:, 1:]), vs.sigma2).T) < TRAJ_TOL
    long_ = vc.vc(tj, X, postfilter=vs)                                               # grows past 256 MiB, released on return
    assert len(tj) == L
    assert ch.same_bits(vc.vc(tj, X[:, :300], postfilter=vs), small), "the 300-frame call after the long one"
    assert ch.same_bits(small, ch.fresh(lambda: vc.vc(make(), X[:, :300], postfilter=vs)))
    long_plain = vc.vc(tj, X)
    assert np.array_equal(long_plain[:, :300], small_plain)
    two = long_plain.copy()
    two[1:] = vc.fvpostf(vs, two[1:])                                                 # (D T doubles in the same scratch: small)
    assert np.array_equal(long_[0], X[0]) and relerr(long_, two) < 1e-13
    assert ch.same_bits(vc.vc(tj, X[:, :300], postfilter=vs), small)
    del long_, long_plain, two, X
    # the frames path with the post-filter
    w, mu, sig = _peaked()
    Tf = 420_000
    assert 2 * 41 * Tf * 8 > 256 << 20
    F = synthdata.sample_frames(4502, w, mu, sig, Tf, 0, 40)
    fm = np.asfortranarray(np.vstack([np.arange(Tf, dtype=np.float64)[None], F.T]))
    vs = vc.VarianceScaling(np.random.default_rng(1).uniform(0.5, 2.0, 40))
    g = vc.GMMMap(*julia_model(w, mu, sig))
    s1 = vc.vc(g, fm[:, :300], postfilter=vs)
    big = vc.vc(g, fm, postfilter=vs)
    assert np.array_equal(big[0], fm[0]) and np.all(np.isfinite(big))
    assert ch.same_bits(vc.vc(g, fm[:, :300], postfilter=vs), s1)
    assert ch.same_bits(s1, ch.fresh(lambda: vc.vc(vc.GMMMap(*julia_model(w, mu, sig)), fm[:, :300], postfilter=vs)))
