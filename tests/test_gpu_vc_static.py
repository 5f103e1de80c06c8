"""GPU: vc of a trajectory converter from STATIC features (bin/vc.jl:75-82 in one call), on device tensors, and with the GV
converter -- vcmi_vc_traj_static, vcmi_vc_traj_dev, vcmi_vc_trajgv, vcmi_vc_trajgv_dev.
The deltas are taken over the whole utterance before it is cut into chunks of length(c) frames (bin/vc.jl:78): the tests hold
the result to the oracle's push_delta -> vc (-> variance_scaling) and show that the per-chunk reading of the deltas is far away.
Tolerances: 1e-6 relative against the oracle for anything behind the trajectory solve (test_gpu_postf.py, test_gpu_gv.py),
1e-12 between two library paths that run the same kernels on the same bytes, equality for the power row."""
import functools

import numpy as np
import pytest

from conftest import julia_model, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-6        # against the oracle
SAME = 1e-12      # between two library paths
CASES = [(260, 100), (90, 100), (101, 100), (2, 100), (1, 100), (20000, 100)]


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _model(Ds, M, seed):
    from oracle import np_oracle as npo
    return npo.synth_model(seed, 4 * Ds, M, lam_lo=1e-3)


@functools.lru_cache(maxsize=None)
def _case(Ds, M, seed, T, L):
    """One utterance and the oracle's reading of it, computed once and shared (read-only):
    static (T,Ds), power (T,), fm_static (Ds+1,T), fm (2Ds+1,T) with the whole-utterance deltas, ref (T,Ds+1) = the oracle's
    vc of it in chunks of L."""
    from oracle import c_oracle as co, np_oracle as npo
    w, mu, sig = _model(Ds, M, seed)
    st = np.cumsum(npo.sample_frames(32, w, mu, sig, T, 0, Ds), axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
    power = np.linspace(0, 1, T)
    X = co.push_delta(st)                                                    # (T, 2Ds): deltas over the whole utterance
    ref = co.TrajectoryGMMMap(co.GMMMap(w, mu, sig)).vc(np.hstack([power[:, None], X]), L)
    return dict(static=_frozen(st), power=_frozen(power), ref=_frozen(ref),
                fm_static=_frozen(np.asfortranarray(np.vstack([power[None], st.T]))),
                fm=_frozen(np.asfortranarray(np.vstack([power[None], X.T]))))


def _traj(vc, Ds, M, seed, L):
    return vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*_model(Ds, M, seed))), L)


def _check_static(vc, Ds, M, seed, T, L, per_chunk):
    from oracle import c_oracle as co
    c = _case(Ds, M, seed, T, L)
    tj = _traj(vc, Ds, M, seed, L)
    out = vc.vc(tj, c["fm_static"], delta=True)
    assert out.shape == (Ds + 1, T) and np.array_equal(out[0], c["power"])
    assert len(tj) == (T - 1) % L + 1                                        # W was left at the last chunk's length
    # the library's own two steps on a fresh converter: host push_delta, then vc of the (2D+1,T) matrix
    two = vc.vc(_traj(vc, Ds, M, seed, L), np.vstack([c["power"][None], vc.push_delta(np.asfortranarray(c["static"].T))]))
    e_lib, e_ref = relerr(out, two), relerr(out, c["ref"].T)
    print(f"static vc Ds={Ds} T={T} L={L}: vs two library steps {e_lib:.2e}, vs oracle {e_ref:.2e}")
    assert e_lib <= SAME and e_ref <= TOL
    if per_chunk and T > L:
        # the other reading -- push_delta on every chunk separately -- is a different result, far outside the tolerance
        Xc = np.vstack([co.push_delta(c["static"][b:b + L]) for b in range(0, T, L)])
        w, mu, sig = _model(Ds, M, seed)
        chunked = co.TrajectoryGMMMap(co.GMMMap(w, mu, sig)).vc(np.hstack([c["power"][:, None], Xc]), L)
        gap = relerr(chunked, c["ref"])
        print(f"   per-chunk deltas vs whole-utterance deltas (oracle): {gap:.2e}")
        assert gap > 1e-3


@pytest.mark.parametrize("T,L", CASES)
def test_static_input_equals_the_reference_pipeline(vc, T, L):
    """vc(tj, fm_static, delta=True) == vc(tj, [power; push_delta(static)]): (101, 100) leaves a one-frame last chunk,
    (20000, 100) is 200 chunks, T <= L is one chunk (both readings of the deltas coincide there)"""
    _check_static(vc, 12, 4, 311, T, L, per_chunk=True)


@pytest.mark.parametrize("T,L", CASES)
def test_static_input_with_the_post_filter(vc, T, L):
    """... followed by fvpostf! over the whole converted matrix, before the download"""
    from oracle import c_oracle as co
    Ds, M, seed = 12, 4, 311
    c = _case(Ds, M, seed, T, L)
    vs = vc.VarianceScaling(np.random.default_rng(2).uniform(0.5, 2.0, Ds))
    tj = _traj(vc, Ds, M, seed, L)
    if T < 2:
        with pytest.raises(vc.DimensionMismatch):                            # the variance of one frame is undefined
            vc.vc(tj, c["fm_static"], postfilter=vs, delta=True)
        assert len(tj) == L                                                  # nothing ran
        return
    out = vc.vc(tj, c["fm_static"], postfilter=vs, delta=True)
    assert out.shape == (Ds + 1, T) and np.array_equal(out[0], c["power"]) and len(tj) == (T - 1) % L + 1
    two = vc.vc(_traj(vc, Ds, M, seed, L), c["fm"], postfilter=vs)          # the (2D+1,T) entry on host-made deltas
    want = co.variance_scaling(np.ascontiguousarray(c["ref"][:, 1:]), vs.sigma2)
    e_lib, e_ref = relerr(out, two), relerr(out[1:], want.T)
    print(f"static vc + post-filter T={T} L={L}: vs the (2D+1,T) entry {e_lib:.2e}, vs oracle {e_ref:.2e}")
    assert e_lib <= SAME and e_ref <= TOL
    with pytest.raises(vc.DimensionMismatch):
        vc.vc(tj, c["fm_static"], postfilter=vc.VarianceScaling(vs.sigma2[:-1]), delta=True)


@pytest.mark.parametrize("Ds,M,seed,T,L", [(40, 8, 640, 150, 64), (13, 3, 311, 50, 20)])
def test_static_input_on_the_other_solver_routes(vc, Ds, M, seed, T, L):
    """static D = 40: the blocked solver's own instantiation at the headline dimension; D = 13 (odd): the padded route"""
    _check_static(vc, Ds, M, seed, T, L, per_chunk=False)


@pytest.mark.parametrize("delta", [True, False])
def test_device_tensors(vc, delta):
    """a CUDA view with a leading dimension in, a CUDA tensor (D+1,T) out, equal to the host-pointer entry's result"""
    import torch
    Ds, M, seed, T, L = 12, 4, 311, 260, 100
    c = _case(Ds, M, seed, T, L)
    fm = c["fm_static"] if delta else c["fm"]
    rows = fm.shape[0]
    wide = np.random.default_rng(5).standard_normal((T, rows + 3))
    wide[:, 1:rows + 1] = fm.T
    dwide = torch.from_numpy(wide).cuda()
    dfm = dwide[:, 1:rows + 1].t()                                           # (rows, T), unit stride along the rows, ld = rows + 3
    assert dfm.stride() == (1, rows + 3)
    vs = vc.VarianceScaling(np.random.default_rng(2).uniform(0.5, 2.0, Ds))
    for pf in (None, vs):
        host = vc.vc(_traj(vc, Ds, M, seed, L), fm, postfilter=pf, delta=delta)
        tj = _traj(vc, Ds, M, seed, L)
        dev = vc.vc(tj, dfm, postfilter=pf, delta=delta)
        assert dev.is_cuda and tuple(dev.shape) == (Ds + 1, T) and dev.stride(0) == 1 and len(tj) == (T - 1) % L + 1
        got = dev.cpu().numpy()
        e = relerr(got, host)
        print(f"device vc delta={delta} postfilter={pf is not None}: vs the host-pointer entry {e:.2e}")
        assert np.array_equal(got[0], c["power"]) and e <= SAME
        assert np.array_equal(dwide.cpu().numpy(), wide)                     # the input is unchanged
    with pytest.raises(vc.DimensionMismatch):
        vc.vc(tj, dfm[:-1], delta=delta)
    # a CPU torch tensor goes the numpy way
    cpu = vc.vc(_traj(vc, Ds, M, seed, L), torch.from_numpy(wide)[:, 1:rows + 1].t(), delta=delta)
    assert isinstance(cpu, np.ndarray) and np.array_equal(cpu, vc.vc(_traj(vc, Ds, M, seed, L), fm, delta=delta))


def _gv_stats(rng, Y):
    """GV mean slightly above the converted track's variance, and a dense SPD GV covariance (the recipe of test_gpu_gv.py)."""
    D = Y.shape[1]
    muv = Y.var(axis=0, ddof=1) * 1.3
    A = rng.standard_normal((D, D))
    return muv, A @ A.T / D * np.mean(muv) ** 2 * 0.1 + np.diag(muv ** 2 * 0.05)


def test_gv_converter(vc):
    """vc(tgv, ...) as one device call: static input, the post-filter, non-default epochs; against fvconvert_gv per chunk of
    the whole-utterance push_delta"""
    import torch
    from oracle import c_oracle as co, np_oracle as npo
    Ds, M, T, L = 12, 4, 70, 30
    w, mu, sig = npo.synth_model(77, 4 * Ds, M, lam_lo=1e-3)
    ref = co.TrajectoryGMMMap(co.GMMMap(w, mu, sig))
    rng = np.random.default_rng(3)
    st = npo.sample_frames(int(rng.integers(1 << 30)), w, mu, sig, T, 0, Ds)
    st = np.cumsum(st, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
    X = co.push_delta(st)
    muv, Sv = _gv_stats(rng, ref.fvconvert(X)[0])
    power = np.linspace(0, 1, T)
    fm_static = np.asfortranarray(np.vstack([power[None], st.T]))
    fm = np.asfortranarray(np.vstack([power[None], X.T]))

    def make():
        return vc.TrajectoryGVGMMMap(vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(w, mu, sig)), L), muv, Sv)

    def want(epochs):
        return np.vstack([ref.fvconvert_gv(X[b:b + L], muv, Sv, epochs, 1.0e-5) for b in range(0, T, L)])   # (T, Ds)

    w100 = want(100)
    tgv = make()
    out = vc.vc(tgv, fm_static, delta=True)
    e = relerr(out[1:], w100.T)
    print(f"GV vc, static input: vs oracle {e:.2e}")
    assert out.shape == (Ds + 1, T) and np.array_equal(out[0], power) and e <= TOL
    assert len(tgv) == 10                                                    # length(tgv) follows the last chunk
    s2 = np.random.default_rng(2).uniform(0.5, 2.0, Ds)
    tgv = make()
    outp = vc.vc(tgv, fm, postfilter=vc.VarianceScaling(s2))
    e = relerr(outp[1:], co.variance_scaling(w100, s2).T)
    print(f"GV vc, (2D+1,T) input + post-filter: vs oracle {e:.2e}")
    assert np.array_equal(outp[0], power) and e <= TOL and len(tgv) == 10
    # the device-tensor form runs the same kernels on the same bytes
    dev = vc.vc(make(), torch.from_numpy(np.ascontiguousarray(fm_static.T)).cuda().t(), delta=True)
    assert dev.is_cuda and relerr(dev.cpu().numpy(), out) <= SAME
    # a chunk of exactly one frame has no variance: T = 61 leaves one
    tgv = make()
    with pytest.raises(vc.DimensionMismatch):
        vc.vc(tgv, fm_static[:, :61], delta=True)
    assert len(tgv) == L
    # non-default epochs reach the kernel
    o20 = make()._vc(fm_static, delta=True, epochs=20)
    e = relerr(o20[1:], want(20).T)
    print(f"GV vc, epochs=20: vs oracle {e:.2e}; vs epochs=100 {relerr(o20, out):.2e}")
    assert e <= TOL and not np.array_equal(o20, out) and relerr(o20, out) > 1e-9


def test_every_converter_type(vc):
    Ds, M, seed, T, L = 12, 4, 311, 90, 100
    c = _case(Ds, M, seed, T, L)
    w, mu, sig = _model(Ds, M, seed)
    g = vc.GMMMap(*julia_model(w, mu, sig))                                  # frame by frame over the 2 Ds = 24 rows
    tj = vc.TrajectoryGMMMap(g, L)
    muv, Sv = _gv_stats(np.random.default_rng(4), c["ref"][:, 1:])
    tgv = vc.TrajectoryGVGMMMap(vc.TrajectoryGMMMap(g, L), muv, Sv)
    rng = np.random.default_rng(2)
    vs, vs2 = vc.VarianceScaling(rng.uniform(0.5, 2.0, Ds)), vc.VarianceScaling(rng.uniform(0.5, 2.0, 2 * Ds))
    assert vc.vc(g, c["fm"], postfilter=vs2).shape == (2 * Ds + 1, T)
    for conv in (tj, tgv):
        out = vc.vc(conv, c["fm"], postfilter=vs)
        assert out.shape == (Ds + 1, T) and np.array_equal(out[0], c["power"]) and np.all(np.isfinite(out))
        assert np.allclose(out[1:].var(axis=1, ddof=1), vs.sigma2, rtol=1e-9)
    with pytest.raises(ValueError, match="delta"):
        vc.vc(g, c["fm"], delta=True)                                        # bin/vc.jl:76 adds deltas for trajectory converters only
    for conv in (vc.TrajectoryGMMMap(g, L), vc.TrajectoryGVGMMMap(vc.TrajectoryGMMMap(g, L), muv, Sv)):
        with pytest.raises(vc.DimensionMismatch):
            vc.vc(conv, c["fm"], delta=True)                                 # (2D+1,T) where static rows are expected
        with pytest.raises(vc.DimensionMismatch):
            vc.vc(conv, c["fm_static"][:-1], delta=True)
        with pytest.raises(vc.DimensionMismatch):
            vc.vc(conv, c["fm_static"], postfilter=vs)                       # static rows where (2D+1,T) is expected
        assert len(conv) == L
