"""The screen kernels' row access in two halves (csrc/gmmmap_rows.hpp: request_frame_rows / finish_frame_rows) and what rests on it in
csrc/gmmmap_screen.hpp: the prologue that requests every tile's rows at clamped positions before it waits for any, the reload of
the rows behind the first survivor's block, and the per-wave survivor bitmap -- on the shapes where each can go wrong: last
workgroups with one live frame, a dead second tile, waves that lie entirely beyond T; rows that are not whole 128-byte lines
(D != DP, an odd leading dimension, a base that is 8- but not 16-byte aligned); survivors that pass the exact test after the
reload; frames of ONE wave that need a second mixture which the other waves of the workgroup do not.

Every frame against the C oracle at the bar of tests/test_gpu_grouping_two_launch.py, 1e-9 relative per frame; every case
twice, bit for bit equal.  A few thousand frames per case (T = 8192 + r: the smallest grouped call and a remainder).
"""
import numpy as np
import pytest

from conftest import julia_model

pytestmark = pytest.mark.gpu

TOL = 1e-9
SORT_MIN = 8192          # kSortMinFrames: the smallest call that is grouped
R_MAX = 127


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
    """frames of the (M, D) peaked model drawn with `weights` (its own by default) and the oracle's answers, built once"""
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


def _convert(vc, g, xt, extra=0, out=None):
    """one device-resident fvconvert of the (D, T) tensor xt with shape 3 (forced where the model's own plan is another one)"""
    from voiceconversion_jl_amd import _lib
    force = extra | (0 if g.convert_plan()[1] == 3 else _lib.DBG_CONVERT_SHAPE_SCREENED)
    _lib.debug_force(force)
    try:
        assert g.convert_plan()[1] == 3
        y = vc.fvconvert(g, xt) if out is None else vc.fvconvert(g, xt, out=out)
        return y.t().cpu().numpy()
    finally:
        _lib.debug_force(0)


def _check(vc, g, X, Yref, extra=0, as_tensor=None, as_out=None):
    """convert twice (bit-equal), every frame against the oracle; as_tensor / as_out build the (D, T) input / output tensors"""
    import torch
    out = []
    for _ in range(2):
        xt = torch.from_numpy(np.array(X)).cuda().t() if as_tensor is None else as_tensor(X)
        out.append(_convert(vc, g, xt, extra, None if as_out is None else as_out(X.shape)))
    Y, Y2 = out
    err = _frame_err(Y, Yref)
    print(f"T = {len(X)}: max per-frame relative error {err.max():.3e} (frame {int(np.argmax(err))})")
    assert np.array_equal(Y, Y2)
    assert np.all(np.isfinite(Y)) and err.max() < TOL, int(np.argmax(err))
    return Y


# ---------------------------------------------------------------- tile edges
@pytest.mark.parametrize("r", [1, 15, 16, 17, 31, 33, 127])
def test_tile_edges_two_tiles(vc, r):
    """128 frames per workgroup, 32 per wave: a last workgroup with one live frame (r = 1), a full tile 0 with a dead tile 1 (16),
    one live frame in tile 1 (17), waves entirely beyond T, whose requests are clamped (all but 127)"""
    from voiceconversion_jl_amd import _lib
    X, Yref = _frames("own64", 64, 40, SORT_MIN + R_MAX)
    T = SORT_MIN + r
    _check(vc, _handle(vc, 64), X[:T], Yref[:T], extra=_lib.DBG_CONVERT_WIDE_TILES)


@pytest.mark.parametrize("r", [1, 15, 17])
def test_tile_edges_one_tile(vc, r):
    """64 frames per workgroup, 16 per wave"""
    X, Yref = _frames("own64", 64, 40, SORT_MIN + R_MAX)
    T = SORT_MIN + r
    _check(vc, _handle(vc, 64), X[:T], Yref[:T])


# ---------------------------------------------------------------- rows that are not whole lines
def test_rows_d38(vc):
    """D = 38, DP = 40: single features, the last k-step reaches beyond D"""
    X, Yref = _frames("d38", 64, 38, SORT_MIN + 17)
    _check(vc, _handle(vc, 64, 38), X, Yref)


@pytest.mark.parametrize("wide", [False, True])
def test_rows_odd_leading_dimension(vc, wide):
    """ldx = ldy = 41 at D = 40: every second row is 8- but not 16-byte aligned"""
    import torch
    from voiceconversion_jl_amd import _lib
    X, Yref = _frames("own64", 64, 40, SORT_MIN + R_MAX)
    T = SORT_MIN + 17

    def as_tensor(X):
        buf = torch.full((len(X), 41), float("nan"), dtype=torch.float64, device="cuda")
        buf[:, :40] = torch.from_numpy(np.array(X)).cuda()
        return buf[:, :40].t()

    def as_out(shape):
        return torch.zeros((shape[0], 41), dtype=torch.float64, device="cuda")[:, :40].t()

    xt = as_tensor(X[:T])
    assert xt.stride() == (1, 41)
    _check(vc, _handle(vc, 64), X[:T], Yref[:T], extra=_lib.DBG_CONVERT_WIDE_TILES if wide else 0, as_tensor=as_tensor, as_out=as_out)


def test_rows_base_not_16_byte_aligned(vc):
    """unpadded rows of D = 40 behind a base that is 8 bytes past a 16-byte boundary"""
    import torch
    X, Yref = _frames("own64", 64, 40, SORT_MIN + R_MAX)
    T = SORT_MIN + 17

    def as_tensor(X):
        flat = torch.empty(X.size + 1, dtype=torch.float64, device="cuda")
        xt = flat[1:].view(len(X), 40)
        xt.copy_(torch.from_numpy(np.array(X)).cuda())
        assert xt.data_ptr() % 16 == 8
        return xt.t()

    def as_out(shape):
        flat = torch.zeros(shape[0] * 40 + 1, dtype=torch.float64, device="cuda")
        return flat[1:].view(shape[0], 40).t()

    _check(vc, _handle(vc, 64), X[:T], Yref[:T], as_tensor=as_tensor, as_out=as_out)


# ---------------------------------------------------------------- survivors that pass the exact test (the reload)
@pytest.mark.parametrize("fp64_screen", [False, True])
def test_trained_model_survivors(vc, fixture_model, fp64_screen):
    """the reference's trained model (M = 32, broad: many mixtures survive the screen and pass the per-wave test) forced to shape
    3, with the bf16 screen (rows of x given up and reloaded for the survivors) and with the FP64 one; each against the oracle
    (their survivor sets differ by terms below e^-46)"""
    import synthdata as sd
    from oracle import c_oracle as co
    from voiceconversion_jl_amd import _lib
    w, mu, sig = fixture_model
    if "trained" not in _REFS:
        X = sd.sample_frames(31, w, mu, sig, SORT_MIN + 17, 0, 40)
        _REFS["trained"] = (X, co.GMMMap(w, mu, sig).fvconvert_mt(X)[0])
    X, Yref = _REFS["trained"]
    g = vc.GMMMap(*julia_model(w, mu, sig))
    for extra in (0, _lib.DBG_CONVERT_WIDE_TILES):
        _check(vc, g, X, Yref, extra=extra | (_lib.DBG_SCREEN_FP64 if fp64_screen else 0))


# ---------------------------------------------------------------- the per-wave survivor rule
KEY_DIMS = 24            # kGroupKeyDims: a frame's group is the nearest source mean over its first 24 features


def _regression(mu, sig, D, m, x):
    """E_m(x) = mu_y + S_yx inv(S_xx) (x - mu_x) (src/gmmmap.jl:109-117)"""
    S = (sig[m] + sig[m].T) / 2.0
    return mu[m, D:] + S[D:, :D] @ np.linalg.solve(S[:D, :D], x - mu[m, :D])


def _points_with_a_runner_up(ref, w, mu, sig, D, g, nats, seed, n=64):
    """Points at which g is the oracle's arg-max and the best other mixture lies exactly `nats` behind it: on the segment from a
    draw of g to a draw of another mixture, where the lead of g over the best other one falls to `nats` (bisection on the
    oracle's log-densities, the construction of oracle/adversarial.py's `imb` frames).  Kept: those whose nearest source mean
    over the key dimensions is g's by a margin (they sort into g's group like the draws around them) and whose y changes by
    more than TOL when the runner-up's term is left out.  Returns (points, runner-up per point)."""
    import synthdata as sd
    from oracle import adversarial as adv
    M = len(w)
    only = np.zeros(M)
    only[g] = 1.0
    Xa = sd.sample_frames(seed, only, mu, sig, n, 0, D)
    others = np.random.default_rng(seed + 1).choice([m for m in range(M) if m != g], n)
    Xb = np.stack([sd.sample_frames(seed + 2 + i, np.eye(M)[m], mu, sig, 1, 0, D)[0] for i, m in enumerate(others)])
    a = np.full(n, g)
    lead = lambda s: adv._lead(ref.logdens(Xa + s[:, None] * (Xb - Xa)), a)          # noqa: E731
    ok = (lead(np.zeros(n)) >= nats) & (lead(np.ones(n)) < nats)
    lo, _ = adv._bisect(lambda s: (lead(s) >= nats) | ~ok, np.zeros(n), np.ones(n), 60)
    P = (Xa + lo[:, None] * (Xb - Xa))[ok]
    L = ref.logdens(P)
    Y = ref.fvconvert(P)
    top, best, second = adv._top2(L)
    L2 = L.copy()
    L2[np.arange(len(P)), top] = -np.inf
    runner = np.argmax(L2, axis=1)
    lse = best + np.log(np.exp(L - best[:, None]).sum(axis=1))
    d2 = ((P[:, None, :KEY_DIMS] - mu[None, :, :KEY_DIMS]) ** 2).sum(axis=2)
    key = np.argmin(d2, axis=1)
    d2o = d2.copy()
    d2o[np.arange(len(P)), key] = np.inf
    keep = []
    for i in range(len(P)):
        pm = np.exp(L[i, runner[i]] - lse[i])
        y_without = (Y[i] - pm * _regression(mu, sig, D, runner[i], P[i])) / (1.0 - pm)
        change = np.linalg.norm(y_without - Y[i]) / np.linalg.norm(Y[i])
        if (top[i] == g and abs(best[i] - second[i] - nats) < 1e-6 and key[i] == g and d2o[i].min() > 1.05 * d2[i, g]
                and change > 2.0 * TOL):
            keep.append(i)
    keep = np.array(keep, dtype=np.int64)
    return P[keep], runner[keep]


@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("g", [5, 33])
def test_one_wave_needs_a_second_mixture(vc, g, wide):
    """every frame a draw of mixture g, so one group holds the call and (the sort being stable) frames 32 w .. 32 w + 31 of a
    128-frame workgroup are wave w's.  Frames 32..63 (wave 1 of the first workgroup) and the call's last frame (alone in its
    workgroup) are replaced by points where g is still the arg-max and ONE other mixture m lies 20 nats behind it: inside the
    e^-46 window, so m must contribute to them -- the oracle's y moves by more than twice TOL when m's term is left out -- and
    to no frame of the waves around them.  A wave bitmap that is not set, or set for another wave, loses that term."""
    from voiceconversion_jl_amd import _lib
    M, D, T = 64, 40, SORT_MIN + 17
    w, mu, sig, ref = _model(M, D)
    name = ("onewave", g)
    if name not in _REFS:
        import synthdata as sd
        P, runner = _points_with_a_runner_up(ref, w, mu, sig, D, g, 20.0, 100 + g)
        assert len(P) >= 8 and len(np.unique(runner)) >= 2, (len(P), runner)
        only = np.zeros(M)
        only[g] = 1.0
        X = sd.sample_frames(17, only, mu, sig, T, 0, D)
        X[32:64] = P[np.arange(32) % len(P)]
        other = np.flatnonzero(runner != runner[0])[0]            # the last frame: a second m
        X[T - 1] = P[other]
        # the frames around them are plain draws of g: g's own by more than the window
        La = ref.logdens(X[:32])
        assert np.all(np.argmax(La, axis=1) == g)
        _REFS[name] = (X, ref.fvconvert_mt(X)[0])
    X, Yref = _REFS[name]
    _check(vc, _handle(vc, M), X, Yref, extra=_lib.DBG_CONVERT_WIDE_TILES if wide else 0)


# ---------------------------------------------------------------- predict
@pytest.mark.parametrize("r", [1, 16, 17, 127])
def test_screened_predict_tile_edges(vc, r):
    """gmmmap_screen_argmax_kernel (two tiles per wave; its prologue is the one-tile screen kernel's) at the same remainders: the
    oracle's arg-max, index for index.  (No entry of the library reports which predict kernel ran: DBG_PREDICT_SCREEN takes the
    screened one for a device input that can be grouped -- at least 8192 frames, at most 1024 mixtures -- which these are.)"""
    import torch
    from voiceconversion_jl_amd import _lib
    X, _ = _frames("own64", 64, 40, SORT_MIN + R_MAX)
    T = SORT_MIN + r
    if "predict" not in _REFS:
        _REFS["predict"] = _model(64)[3].predict(X)
    want = _REFS["predict"][:T]
    g = _handle(vc, 64)
    got = []
    _lib.debug_force(_lib.DBG_PREDICT_SCREEN)
    try:
        for _ in range(2):
            got.append(np.asarray(vc.predict(g.px, torch.from_numpy(np.array(X[:T])).cuda().t()).cpu()))
    finally:
        _lib.debug_force(0)
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(got[0], want)
