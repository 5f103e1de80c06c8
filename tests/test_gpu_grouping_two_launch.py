"""fvconvert's frame grouping in two launches (csrc/gmmmap_group.hip: key kernel with chunk and super-chunk histograms, then
gmmmap_group_place_kernel) and the screen kernels that take their groups from gbase (csrc/gmmmap_screen.hpp: groups_in_range),
on the shapes where that can go wrong: the smallest grouped call, partial last chunks and tiles, two super-chunks, models whose
frames leave most groups empty (runs of equal gbase entries, first, last and in between), many small groups per workgroup,
more groups than lanes and more than one bitmap word, four groups, one group -- and the two super-chunk tables, which must be
zero again for every call on a handle.

Every frame against the C oracle (src/gmmmap.jl:109-117) at the bar of tests/test_gpu_adversarial.py, 1e-9 relative per frame;
twice, bit for bit equal: the sort is stable, so the result is a function of the data alone.  Frames are draws from the synthetic
peaked model's own p(x), a few thousand per case.
"""
import numpy as np
import pytest

from conftest import julia_model

pytestmark = pytest.mark.gpu

TOL = 1e-9
SORT_MIN = 8192          # kSortMinFrames: the smallest call that is grouped
SMALL_CALL = 32768       # kSmallCallFrames: above it a wave holds two frame tiles


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


_MODELS = {}
_REFS = {}


def _model(M, D=40):
    if (M, D) not in _MODELS:
        import synthdata as sd
        from oracle import c_oracle as co
        w, mu, sig = sd.synth_model(1002, 2 * D, M, lam_lo=1e-5)
        _MODELS[(M, D)] = (w, mu, sig, co.GMMMap(w, mu, sig))
    return _MODELS[(M, D)]


def _frames(name, M, D, T, weights=None, seed=13):
    """frames of the (M, D) model drawn with `weights` (the model's own by default) and the oracle's answers, built once"""
    if name not in _REFS:
        import synthdata as sd
        w, mu, sig, ref = _model(M, D)
        X = sd.sample_frames(seed, w if weights is None else weights, mu, sig, T, 0, D)
        _REFS[name] = (X, ref.fvconvert_mt(X)[0])
    X, Yref = _REFS[name]
    X.setflags(write=False)
    Yref.setflags(write=False)
    return X, Yref


def _frame_err(Y, Yref):
    return np.linalg.norm(Y - Yref, axis=1) / np.maximum(np.linalg.norm(Yref, axis=1), 1e-300)


def _handle(vc, M, D=40):
    w, mu, sig, _ = _model(M, D)
    return vc.GMMMap(*julia_model(w, mu, sig))


def _convert(vc, g, X, extra=0):
    """one device-resident fvconvert with shape 3 (forced where the model's own plan is another one)"""
    import torch
    from voiceconversion_jl_amd import _lib
    force = extra | (0 if g.convert_plan()[1] == 3 else _lib.DBG_CONVERT_SHAPE_SCREENED)
    _lib.debug_force(force)
    try:
        assert g.convert_plan()[1] == 3
        return vc.fvconvert(g, torch.from_numpy(np.array(X)).cuda().t()).t().cpu().numpy()
    finally:
        _lib.debug_force(0)


def _check(vc, g, X, Yref, extra=0):
    Y = _convert(vc, g, X, extra)
    Y2 = _convert(vc, g, X, extra)
    err = _frame_err(Y, Yref)
    print(f"T = {len(X)}: max per-frame relative error {err.max():.3e}")
    assert np.array_equal(Y, Y2)
    assert np.all(np.isfinite(Y)) and err.max() < TOL, int(np.argmax(err))
    return Y


@pytest.mark.parametrize("T", [SORT_MIN, SORT_MIN + 17, 33_000])
def test_sizes(vc, T):
    """exactly kSortMinFrames; a partial last chunk and tile; above kSmallCallFrames (two tiles per wave) with 33 chunks = two
    super-chunks of 32"""
    assert SORT_MIN + 17 < SMALL_CALL < 33_000
    X, Yref = _frames("own64", 64, 40, 33_000)
    _check(vc, _handle(vc, 64), X[:T], Yref[:T])


def test_fp64_key_kernel(vc):
    """gmmmap_group_key_kernel fills the same tables as the bf16 one"""
    from voiceconversion_jl_amd import _lib
    X, Yref = _frames("own64", 64, 40, 33_000)
    T = SORT_MIN + 17
    _check(vc, _handle(vc, 64), X[:T], Yref[:T], extra=_lib.DBG_GROUP_KEY_FP64)


def _only(M, mixtures):
    w = np.zeros(M)
    w[list(mixtures)] = 1.0 / len(mixtures)
    return w


@pytest.mark.parametrize("mixtures", [(0, 31, 63), (17, 18, 40), (61, 62, 63)])
def test_three_mixtures_of_64(vc, mixtures):
    """61 empty groups: before, between and after the three that hold the frames"""
    X, Yref = _frames(("three", mixtures), 64, 40, SORT_MIN + 17, weights=_only(64, mixtures))
    _check(vc, _handle(vc, 64), X, Yref)


def test_many_small_groups(vc):
    """60 groups of about 5-40 frames and four large ones: a workgroup of 64 positions holds three or more groups wherever the
    small ones lie (the range test of the `keys` bitmap)"""
    M, T = 64, SORT_MIN
    small = np.array([5 + (7 * m) % 36 for m in range(M)], dtype=float)       # 5 .. 40 frames
    small[[0, 21, 42, 63]] = 0.0
    w = small.copy()
    w[[0, 21, 42, 63]] = (T - small.sum()) / 4.0
    X, Yref = _frames("small", M, 40, T, weights=w / w.sum())
    _check(vc, _handle(vc, M), X, Yref)


def test_200_mixtures_d24(vc):
    """more groups than lanes in the prefix, seven bitmap words, four turns of the group search"""
    X, Yref = _frames("m200", 200, 24, SORT_MIN + 17)
    _check(vc, _handle(vc, 200, 24), X, Yref)


def test_four_mixtures(vc):
    """the smallest groupable model"""
    X, Yref = _frames("m4", 4, 40, SORT_MIN + 17)
    _check(vc, _handle(vc, 4), X, Yref)


def test_identical_frames(vc):
    """one group holds everything"""
    X0, Y0 = _frames("own64", 64, 40, 33_000)
    X = np.repeat(X0[5:6], SORT_MIN + 17, axis=0)
    Y = _check(vc, _handle(vc, 64), X, np.repeat(Y0[5:6], len(X), axis=0))
    assert np.all(Y == Y[0])


def test_screened_predict_three_mixtures(vc):
    """gmmmap_screen_argmax_kernel shares the prologue: the oracle's predict, index for index"""
    import torch
    from voiceconversion_jl_amd import _lib
    mixtures = (17, 18, 40)
    X, _ = _frames(("three", mixtures), 64, 40, SORT_MIN + 17, weights=_only(64, mixtures))
    ref = _model(64)[3]
    g = _handle(vc, 64)
    _lib.debug_force(_lib.DBG_PREDICT_SCREEN)
    try:
        idx = np.asarray(vc.predict(g.px, torch.from_numpy(np.array(X)).cuda().t()).cpu())
    finally:
        _lib.debug_force(0)
    want = ref.predict(X)
    assert set(np.unique(want)) == {m + 1 for m in mixtures}
    assert np.array_equal(idx, want)


def test_calls_of_different_length_on_one_handle(vc):
    """33 chunks (two super-chunk rows), 9 chunks (one), and both again: each call finds its super-chunk table zero, whatever
    the call before the last one left in it"""
    X, Yref = _frames("own64", 64, 40, 33_000)
    g = _handle(vc, 64)
    out = []
    for T in (33_000, SORT_MIN + 17, 33_000, SORT_MIN + 17):
        Y = _convert(vc, g, X[:T])
        err = _frame_err(Y, Yref[:T])
        print(f"T = {T}: max per-frame relative error {err.max():.3e}")
        assert err.max() < TOL, (T, int(np.argmax(err)))
        out.append(Y)
    assert np.array_equal(out[0], out[2]) and np.array_equal(out[1], out[3])
