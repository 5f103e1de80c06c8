"""GPU: vc_batch -- vc over a whole list of utterances in one call (vcmi_vc_frames_batch, vcmi_vc_traj_batch, vcmi_vc_trajgv_batch
and the two *_batch_dev forms; csrc/vc_batch.hip).  The rule under test: vc_batch(c, fms, ...)[u] is what vc(c_u, fms[u], ...)
returns for a fresh converter c_u with len(c_u) = len(c).
Bars: equality for the power row; bit for bit (np.array_equal) between the batch and the loop of a trajectory converter
(fvconvert_batch is held bit-identical to fvconvert by test_gpu_trajectory.py / test_gpu_traj_em.py, and the batch's end kernels
keep the single call's summation order); SAME = 1e-12 between two library paths; 1e-6 against the oracle behind a trajectory
solve; 1e-9 against the oracle frame by frame.  Models and helpers: tests/test_gpu_vc_static.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import julia_model, relerr
from test_gpu_vc_static import _case, _gv_stats, _model, _traj

pytestmark = pytest.mark.gpu
TOL = 1e-6        # against the oracle, behind a trajectory solve
TOL_FRAMES = 1e-9  # against the oracle, frame by frame
SAME = 1e-12      # between two library paths
MODELS = {"main": (12, 4, 311, 20), "own": (40, 8, 640, 64), "padded": (13, 3, 311, 20)}   # Ds, M, seed, L
RAGGED = [0, 1, 2, 19, 20, 21, 41, 60, 100]


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    m.set_devices([])
    return m


def _sigma2(Ds):
    return np.random.default_rng(2).uniform(0.5, 2.0, Ds)


def _fm(Ds, M, seed, T, L, static):
    """utterance of T frames of the shared cases (T = 0: an empty matrix)"""
    if T == 0:
        return np.zeros(((Ds if static else 2 * Ds) + 1, 0), order="F")
    return _case(Ds, M, seed, T, L)["fm_static" if static else "fm"]


def _oracle(Ds, M, seed, T, L, s2):
    """(Ds+1, T): the oracle's push_delta -> vc in chunks of L (-> variance_scaling over the utterance)"""
    from oracle import c_oracle as co
    ref = _case(Ds, M, seed, T, L)["ref"]
    if s2 is not None:
        ref = np.hstack([ref[:, :1], co.variance_scaling(np.ascontiguousarray(ref[:, 1:]), s2)])
    return ref.T


def _check_against_loop(vc, name, Ts, static, filt, make=None, bits=True, oracle=True, **kw):
    Ds, M, seed, L = MODELS[name]
    make = make or (lambda: _traj(vc, Ds, M, seed, L))
    s2 = _sigma2(Ds) if filt else None
    vs = vc.VarianceScaling(s2) if filt else None
    fms = [_fm(Ds, M, seed, T, L, static) for T in Ts]
    c = make()
    outs = vc.vc_batch(c, fms, postfilter=vs, delta=static, **kw)
    assert len(c) == L and len(outs) == len(Ts)                              # the batch leaves len(c) alone
    for T, fm, out in zip(Ts, fms, outs):
        assert out.shape == (Ds + 1, T) and out.flags.f_contiguous
        if T == 0:
            continue
        single = make()
        want = single._vc(fm, vs, delta=static, **kw) if kw else vc.vc(single, fm, postfilter=vs, delta=static)
        e_loop = relerr(out, want)
        assert np.array_equal(out[0], fm[0])                                 # the power row, bit for bit
        if oracle:
            e_ref = relerr(out, _oracle(Ds, M, seed, T, L, s2))
            print(f"{name} static={static} filter={filt} T={T}: vs the loop {e_loop:.2e}, vs the oracle {e_ref:.2e}")
            assert e_ref <= TOL
        assert e_loop <= SAME
        if bits:
            assert np.array_equal(out, want), f"T={T}: the batch is not the loop's result bit for bit ({e_loop:.2e})"
    return outs


@pytest.mark.parametrize("filt", [False, True])
@pytest.mark.parametrize("static", [True, False])
@pytest.mark.parametrize("name", list(MODELS))
def test_batch_equals_the_loop_trajectory(vc, name, static, filt):
    """one ragged batch (empty, one-frame, L-1, L, L+1, 2L+1 ... utterances) == vc on a fresh converter per utterance, bit for
    bit, and the oracle's push_delta -> vc -> variance_scaling per utterance; the filter cases run without the T = 1 utterance"""
    _check_against_loop(vc, name, [T for T in RAGGED if not (filt and T == 1)], static, filt)


@pytest.mark.parametrize("name", list(MODELS))
def test_gv_converter(vc, name):
    """the GV converter over the same batch without the lengths that leave a one-frame chunk, epochs = 4, static input and the
    filter: bit for bit against the loop"""
    Ds, M, seed, L = MODELS[name]
    muv, Sv = _gv_stats(np.random.default_rng(4), _case(Ds, M, seed, 100, L)["ref"][:, 1:])

    def make():
        return vc.TrajectoryGVGMMMap(_traj(vc, Ds, M, seed, L), muv, Sv)

    Ts = [T for T in RAGGED if T % L != 1]
    assert 0 in Ts and 2 in Ts and 100 in Ts
    _check_against_loop(vc, name, Ts, True, True, make=make, oracle=False, epochs=4)
    _check_against_loop(vc, name, Ts, False, False, make=make, oracle=False, epochs=4)


def test_em_per_chunk(vc):
    """em_iters = 2 on the small model: the handle's setting is honoured per chunk.  Bit for bit against the loop: with EM on,
    tests/test_gpu_traj_em.py::test_parity_with_the_restatement already holds the batch call equal to the single call bit for
    bit (np.array_equal of fvconvert_batch and fvconvert, the shortest utterance alone included), and
    test_vc_runs_em_per_chunk holds vc to fvconvert per chunk the same way -- so the bar here is equality, not SAME."""
    Ds, M, seed, L = MODELS["main"]

    def make():
        t = _traj(vc, Ds, M, seed, L)
        t.em_iters = 2
        return t

    Ts = [T for T in RAGGED if T != 1]
    _check_against_loop(vc, "main", Ts, True, True, make=make, oracle=False)
    c = make()
    vc.vc_batch(c, [_fm(Ds, M, seed, T, L, True) for T in Ts], delta=True)
    assert len(c.em_history()) == 2 and np.all(np.isfinite(c.em_history()))   # the call ran two E-steps


@functools.lru_cache(maxsize=None)
def _frames_case():
    """GMMMap over the 2 Ds = 24 rows of the main model: 300 utterances of 2..7 frames (more than the device has CUs) and three
    that cross the 2048-frame chunk of the statistics; the oracle's vc of each, computed once"""
    from oracle import c_oracle as co, np_oracle as npo
    Ds, M, seed, _ = MODELS["main"]
    w, mu, sig = _model(Ds, M, seed)
    D = 2 * Ds
    rng = np.random.default_rng(77)
    Ts = [int(t) for t in rng.integers(2, 8, 300)] + [2048, 2049, 4097]
    N = sum(Ts)
    X = npo.sample_frames(78, w, mu, sig, N, 0, D)                           # (N, D)
    fm_all = np.hstack([rng.standard_normal((N, 1)), X])                     # (N, D+1)
    ref_all = co.GMMMap(w, mu, sig).vc(fm_all)
    first = np.concatenate([[0], np.cumsum(Ts)])
    fms = [np.asfortranarray(fm_all[a:b].T) for a, b in zip(first[:-1], first[1:])]
    refs = [ref_all[a:b].T for a, b in zip(first[:-1], first[1:])]
    for a in fms + refs:
        a.setflags(write=False)
    return fms, refs


def test_frame_by_frame(vc):
    fms, refs = _frames_case()
    Ds, M, seed, _ = MODELS["main"]
    D = 2 * Ds
    g = vc.GMMMap(*julia_model(*_model(Ds, M, seed)))
    assert len(fms) > 256
    plain = vc.vc_batch(g, fms)
    vs = vc.VarianceScaling(_sigma2(D))
    filt = vc.vc_batch(g, fms, postfilter=vs)
    assert len(plain) == len(filt) == len(fms)
    worst = dict(loop=0.0, loop_f=0.0, ref=0.0)
    for fm, ref, p, f in zip(fms, refs, plain, filt):
        assert p.shape == fm.shape == f.shape
        assert np.array_equal(p[0], fm[0]) and np.array_equal(f[0], fm[0])   # the power rows
        worst["loop"] = max(worst["loop"], relerr(p, vc.vc(g, fm)))
        worst["loop_f"] = max(worst["loop_f"], relerr(f, vc.vc(g, fm, postfilter=vs)))
        worst["ref"] = max(worst["ref"], relerr(p, ref))
        # the filter's own arithmetic, to the bits: fvpostf per utterance on the unfiltered batch result
        assert np.array_equal(f[1:], vc.fvpostf(vs, np.asfortranarray(p[1:]))), fm.shape
    print(f"frame by frame, {len(fms)} utterances: vs the loop {worst['loop']:.2e} (filtered {worst['loop_f']:.2e}), vs the oracle {worst['ref']:.2e}")
    assert worst["loop"] <= SAME and worst["loop_f"] <= SAME and worst["ref"] <= TOL_FRAMES
    assert vc.vc_batch(g, []) == []
    with pytest.raises(ValueError, match="delta"):
        vc.vc_batch(g, fms[:2], delta=True)
    with pytest.raises(vc.DimensionMismatch):
        vc.vc_batch(g, [fms[0], fms[1][:-1]])
    with pytest.raises(vc.DimensionMismatch):
        vc.vc_batch(g, [fms[0], fms[1][:, :1]], postfilter=vs)               # the variance of one frame is undefined


def test_trajectory_over_the_statistics_chunk(vc):
    """a 4097-frame utterance (three 2048-frame statistics items, 42 chunks of L = 100) beside a 2-frame one, with the filter"""
    Ds, M, seed, _ = MODELS["main"]
    L = 100
    vs = vc.VarianceScaling(_sigma2(Ds))
    fms = [_case(Ds, M, seed, 4097, L)["fm_static"], _case(Ds, M, seed, 2, L)["fm_static"]]
    c = _traj(vc, Ds, M, seed, L)
    outs = vc.vc_batch(c, fms, postfilter=vs, delta=True)
    assert len(c) == L
    for fm, out, T in zip(fms, outs, (4097, 2)):
        want = vc.vc(_traj(vc, Ds, M, seed, L), fm, postfilter=vs, delta=True)
        e = relerr(out, _oracle(Ds, M, seed, T, L, vs.sigma2))
        print(f"T={T}: vs the loop {relerr(out, want):.2e}, vs the oracle {e:.2e}")
        assert np.array_equal(out[0], fm[0]) and np.array_equal(out, want) and e <= TOL


def test_device_tensors(vc):
    """a list of device tensors in (one of them a view with a leading dimension), device tensors out: SAME against the host
    entry; then on a non-default stream, followed by a second call on another stream with no host synchronisation between
    them (the scratch order, as tests/test_gpu_call_history.py holds it for the other _dev families)"""
    import torch
    Ds, M, seed, L = MODELS["main"]
    vs = vc.VarianceScaling(_sigma2(Ds))
    Ts = [0, 2, 19, 21, 41, 100]
    rng = np.random.default_rng(5)

    def device_list(static):
        out = []
        for k, T in enumerate(Ts):
            fm = _fm(Ds, M, seed, T, L, static)
            if k == 3:                                                       # not dense: ld = rows + 3
                wide = rng.standard_normal((T, fm.shape[0] + 3))
                wide[:, 1:fm.shape[0] + 1] = fm.T
                out.append(torch.from_numpy(wide).cuda()[:, 1:fm.shape[0] + 1].t())
            else:
                out.append(torch.from_numpy(np.array(fm.T, order="C")).cuda().t())
        return out

    results = {}
    for static in (True, False):
        for pf in (None, vs):
            host = vc.vc_batch(_traj(vc, Ds, M, seed, L), [_fm(Ds, M, seed, T, L, static) for T in Ts], postfilter=pf, delta=static)
            c = _traj(vc, Ds, M, seed, L)
            dfms = device_list(static)
            devs = vc.vc_batch(c, dfms, postfilter=pf, delta=static)
            assert len(c) == L
            for T, h, d, dfm in zip(Ts, host, devs, dfms):
                assert d.is_cuda and tuple(d.shape) == (Ds + 1, T)
                got = d.cpu().numpy()
                assert relerr(got, h) <= SAME if T else got.size == 0
                if T:
                    assert np.array_equal(got[0], dfm.cpu().numpy()[0])
            results[static, pf is not None] = [d.cpu().numpy() for d in devs]
    with pytest.raises(TypeError):
        vc.vc_batch(_traj(vc, Ds, M, seed, L), [device_list(True)[1], _fm(Ds, M, seed, 2, L, True)], delta=True)
    with pytest.raises(vc.DimensionMismatch):
        vc.vc_batch(_traj(vc, Ds, M, seed, L), device_list(False), delta=True)
    # two streams, one converter, one thread: call A on s1, call B on s2 right behind it
    c = _traj(vc, Ds, M, seed, L)
    A, B = device_list(True), device_list(False)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for r in range(2):
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            a = vc.vc_batch(c, A, postfilter=vs, delta=True)
        with torch.cuda.stream(s2):
            b = vc.vc_batch(c, B, postfilter=vs, delta=False)
        torch.cuda.synchronize()
        for got, want in zip(a, results[True, True]):
            assert np.array_equal(got.cpu().numpy(), want), f"round {r}: call A on stream 1"
        for got, want in zip(b, results[False, True]):
            assert np.array_equal(got.cpu().numpy(), want), f"round {r}: call B on stream 2"


def test_refusals_leave_everything_untouched(vc):
    """every refusal of include/vcmi.h comes before anything is uploaded or launched: the output buffers keep their fill
    pattern, len(c) is what it was, and a good call afterwards gives the right answer"""
    from voiceconversion_jl_amd import _lib
    Ds, M, seed, L = MODELS["main"]
    s2 = _sigma2(Ds)
    FILL = -7.25
    dpp = C.POINTER(C.c_double)

    def raw(entry, h, Ts, static, sigma2, extra=()):
        """the C entry on sentinel-filled outputs -> (status, untouched?)"""
        fms = [np.asfortranarray(_fm(Ds, M, seed, max(T, 0), L, static)) for T in Ts]
        outs = [np.full((Ds + 1, max(T, 1)), FILL, order="F") for T in Ts]
        n = len(Ts)
        T = np.array(Ts, dtype=np.int64)
        rc = entry(h, n, (dpp * n)(*[_lib.dptr(f) for f in fms]), _lib.iptr(T), int(static), *extra,
                   None if sigma2 is None else _lib.dptr(sigma2), (dpp * n)(*[_lib.dptr(o) for o in outs]))
        return rc, all(np.all(o == FILL) for o in outs)

    tj = _traj(vc, Ds, M, seed, L)
    traj = _lib.lib.vcmi_vc_traj_batch
    # a post-filter with some T_u = 1
    assert raw(traj, tj._h, [20, 1, 41], True, s2) == (_lib.VCMI_ERR_DIM, True) and len(tj) == L
    with pytest.raises(vc.DimensionMismatch):
        vc.vc_batch(tj, [_fm(Ds, M, seed, T, L, True) for T in (20, 1)], postfilter=vc.VarianceScaling(s2), delta=True)
    # a row count that does not fit the converter, sigma2 of the wrong length
    with pytest.raises(vc.DimensionMismatch):
        vc.vc_batch(tj, [_fm(Ds, M, seed, 20, L, True), _fm(Ds, M, seed, 19, L, False)], delta=True)
    with pytest.raises(vc.DimensionMismatch):
        vc.vc_batch(tj, [_fm(Ds, M, seed, 20, L, True)], postfilter=vc.VarianceScaling(s2[:-1]), delta=True)
    assert len(tj) == L
    # a GV converter with a one-frame chunk in any utterance; over a handle with EM on
    muv, Sv = _gv_stats(np.random.default_rng(4), _case(Ds, M, seed, 100, L)["ref"][:, 1:])
    tgv = vc.TrajectoryGVGMMMap(_traj(vc, Ds, M, seed, L), muv, Sv)
    gv = _lib.lib.vcmi_vc_trajgv_batch
    assert raw(gv, tgv._h, [20, 41, 19], True, None, extra=(4, 1.0e-5)) == (_lib.VCMI_ERR_DIM, True) and len(tgv) == L
    tgv.tgmm.em_iters = 1
    assert raw(gv, tgv._h, [20, 19], True, None, extra=(4, 1.0e-5)) == (_lib.VCMI_ERR_ARG, True) and len(tgv) == L
    tgv.tgmm.em_iters = 0
    # length(c) < 1
    t0 = _traj(vc, Ds, M, seed, 0)
    assert raw(traj, t0._h, [20, 19], True, None) == (_lib.VCMI_ERR_ARG, True) and len(t0) == 0
    # negative counts and lengths
    assert raw(traj, tj._h, [20, -1], True, None)[0] == _lib.VCMI_ERR_ARG
    # the frame-by-frame entry
    g = vc.GMMMap(*julia_model(*_model(Ds, M, seed)))
    fms = [np.asfortranarray(np.random.default_rng(9).standard_normal((2 * Ds + 1, T))) for T in (3, 1)]
    outs = [np.full(f.shape, FILL, order="F") for f in fms]
    s2g = _sigma2(2 * Ds)
    rc = _lib.lib.vcmi_vc_frames_batch(g._h, 2, (dpp * 2)(*[_lib.dptr(f) for f in fms]), _lib.iptr(np.array([3, 1], dtype=np.int64)),
                                       _lib.dptr(s2g), (dpp * 2)(*[_lib.dptr(o) for o in outs]))
    assert rc == _lib.VCMI_ERR_DIM and all(np.all(o == FILL) for o in outs)
    # n = 0 is a no-op; after the refusals the same handles convert correctly
    assert vc.vc_batch(tj, []) == [] and traj(tj._h, 0, None, None, 1, None, None) == _lib.VCMI_OK
    for conv, kw in ((tj, {}), (tgv, dict(epochs=4))):
        fm = _fm(Ds, M, seed, 41 if conv is tj else 60, L, True)
        out = vc.vc_batch(conv, [fm], postfilter=vc.VarianceScaling(s2), delta=True, **kw)[0]
        fresh = _traj(vc, Ds, M, seed, L) if conv is tj else vc.TrajectoryGVGMMMap(_traj(vc, Ds, M, seed, L), muv, Sv)
        want = fresh._vc(fm, vc.VarianceScaling(s2), delta=True, **kw)
        assert np.array_equal(out, want) and len(conv) == L
