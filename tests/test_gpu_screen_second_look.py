"""The second look of the bf16 screen (csrc/gmmmap_screen.hpp, step 2): a mixture that its four strongest rows leave open for
some frame of a wave is looked at with its sixteen strongest rows, in the wave, before it becomes a survivor.

What the look is FOR is a count: on draws of the peaked M = 64, D = 40 model the four rows let a wrong mixture through in about
every second workgroup (every one of them is then whitened in FP64 by the owning waves, fails the exact test and is thrown away),
the sixteen rows none.  Two bounds on the FP64 MFMAs of one call (`convert_plan()[0]`):

    issued <= 4 FT 42 (sum over workgroups of K_w + 2)                      the issue's
    issued <= base + 2 (4 FT 42)                                             the one that tells a working look from none

K_w = distinct group keys among the workgroup's sorted positions, the groups recomputed here (nearest source mean over the first
24 features, stable sort); + 2 for two frames whose bf16 key differs from the exact nearest mean.  The first bound charges every
key 42 MFMAs on all 4 FT tiles of its workgroup.  That is generous: the keys after the first go through the per-wave test and cost
a wave whose frames do not need them 22 per tile, so the bound leaves 2,156 MFMAs of room at one tile per wave and 4,712 at two --
at two that is more than ALL the survivors' whitening (2,860): the parent issues 43,616 there and passes 43,680.  Alone it proves
nothing at two tiles per wave, the benchmark's instantiation.  So the test replays the kernel's steps 1 and 3 in numpy as well:
`base` = 42 per tile for the first key of a workgroup in every wave, and for every further key, in index order, 22 or 42 per
tile and wave by the per-wave test against the running maximum (30,268 and 38,968; the kernel's own count on these frames
is exactly that with the look, and base + the replayed survivors' whitening without it: 5,104 at one tile per wave, where every
wave whitens a survivor, 2,860 at two, where the waves that own it do).  The allowance is the issue's "+ 2" in its own unit, two
mixtures on a whole workgroup.  That THIS bound says something is asserted, not assumed: the survivors' replayed whitening must be
more than four times the allowance (15 x and 4.3 x on these frames), so the parent, or a build whose look is inert, fails it at
either width.  (The issue asked for 44 n4 > ten times the slack; with n4 = 58 / 49 four-row survivors that is 2,552 / 2,156 and
holds for no reading of "slack" that covers the room the first bound really leaves, which is what this replaces.)

T = 8192 + 17 leaves ONE frame in the last tile: its other fifteen columns carry x = 0, which is no frame -- about forty mixtures
pass every bound for it, and a kernel that screens those columns whitens them all in the last workgroup (3,496 MFMAs at one
tile per wave, 1,788 at two: measured on the parent), which neither bound allows at one tile per wave.

The frames are the first T of the 8192 + 127 draws of `sample_frames(13, ...)` that tests/test_gpu_screen_round_trips.py uses --
deliberately the prefix of the longer draw, not `sample_frames(13, ..., T)`, which draws other frames: the prefix is what the
issue's replay figures (0.45 four-row survivors per 64-frame workgroup, 0.75 per 128-frame one: 58 and 49) belong to.

Every frame against the C oracle at 1e-9, as tests/test_gpu_screen_round_trips.py; two calls bit for bit equal.  And the same
frames with every feature shifted by -2000, where the margins of the bf16 bounds grow (c_i = P_i mu is thousands of times the
a_i that decide): y of shape 3 against the dense loop at 1e-13 per frame, no statement about the count.

That the look never rules out a real runner-up is what test_one_wave_needs_a_second_mixture, test_trained_model_survivors and
tests/test_gpu_adversarial.py check; tests/test_screen2_host.py checks the bound itself on the CPU.
"""
import numpy as np
import pytest

from conftest import julia_model

pytestmark = pytest.mark.gpu

TOL = 1e-9
M, D = 64, 40
T = 8192 + 17
KEY_DIMS = 24            # kGroupKeyDims
PER_PAIR = 42            # FP64 MFMAs per (16-frame tile, mixture) at D = 40: 22 whitening + 20 regression k-steps
PRUNE = 46.0


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


_CACHE = {}


def _case():
    """model, frames (the first T of the 8192 + 127 draws tests/test_gpu_screen_round_trips.py uses), the oracle's y; built once"""
    if "case" not in _CACHE:
        import synthdata as sd
        from oracle import c_oracle as co
        w, mu, sig = sd.synth_model(1002, 2 * D, M)
        X = sd.sample_frames(13, w, mu, sig, 8192 + 127, 0, D)[:T].copy()
        Yref = co.GMMMap(w, mu, sig).fvconvert_mt(X)[0]
        X.setflags(write=False)
        Yref.setflags(write=False)
        _CACHE["case"] = (w, mu, sig, X, Yref)
    return _CACHE["case"]


def _replay():
    """per frame in sorted order: its key, the exact log-densities and the certified four-row bounds of every mixture"""
    if "replay" not in _CACHE:
        w, mu, sig, X, _ = _case()
        mux = mu[:, :D]
        d2 = (X[:, :KEY_DIMS] ** 2).sum(1)[:, None] - 2.0 * X[:, :KEY_DIMS] @ mux[:, :KEY_DIMS].T + (mux[:, :KEY_DIMS] ** 2).sum(1)[None]
        key = np.argmin(d2, axis=1)
        perm = np.argsort(key, kind="stable")
        Xs, ks = X[perm], key[perm]
        nx = np.linalg.norm(Xs, axis=1)
        L = np.empty((T, M))
        B4 = np.empty((T, M))
        for m in range(M):
            lam, V = np.linalg.eigh(sig[m][:D, :D])                   # ascending: the first columns are the strongest rows
            lc = np.log(w[m]) - 0.5 * np.sum(np.log(lam)) - 0.5 * D * np.log(2.0 * np.pi)
            P = V / np.sqrt(lam)
            A = (Xs - mux[m]) @ P
            eps = 2.0 ** -12 * (np.linalg.norm(P, axis=0)[None] * nx[:, None] + np.abs(mux[m] @ P)[None])
            Ac = np.maximum(np.abs(A) - eps, 0.0)
            L[:, m] = lc - 0.5 * (A ** 2).sum(1)
            B4[:, m] = lc - 0.5 * (Ac[:, :4] ** 2).sum(1)
        _CACHE["replay"] = (ks, L, B4)
    return _CACHE["replay"]


def _replayed_counts(FT):
    """The kernel's steps 1 and 3 on the replayed groups, 64 FT frames per workgroup, 16 FT per wave:
    (sum over the workgroups of K_w, base = FP64 MFMAs of the workgroups' keys, four-row survivors, their whitening's MFMAs)"""
    ks, L, B4 = _replay()
    per_wg, per_wave = 64 * FT, 16 * FT
    sum_k = base = n4 = whitening = 0
    for p0 in range(0, T, per_wg):
        sl = slice(p0, min(T, p0 + per_wg))
        n = sl.stop - sl.start
        keys = np.unique(ks[sl])
        sum_k += len(keys)
        run = np.full(per_wg, -np.inf)                                # running maximum per column; columns beyond T stay out
        run[:n] = L[sl][:, keys[0]]
        base += 4 * FT * PER_PAIR                                     # the first key: whitening and regression in every wave
        for k in keys[1:]:                                            # the others in index order, per-wave test after the whitening
            l = np.full(per_wg, -np.inf)
            l[:n] = L[sl][:, k]
            for v in range(4):
                cols = slice(v * per_wave, (v + 1) * per_wave)
                go = bool(np.any(l[cols] > run[cols] - PRUNE))
                base += FT * (PER_PAIR if go else 22)
                if go:
                    run[cols] = np.maximum(run[cols], l[cols])
        open_ = B4[sl] > (run[:n] - PRUNE)[:, None]
        open_[:, keys] = False
        for m in np.flatnonzero(open_.any(axis=0)):
            n4 += 1
            owners = sum(bool(open_[v * per_wave:(v + 1) * per_wave, m].any()) for v in range(4))
            whitening += 22 * FT * (owners if FT == 2 else 4)         # one tile per wave: no per-wave bitmap, every wave whitens
    return sum_k, base, n4, whitening


def _frame_err(Y, Yref):
    return np.linalg.norm(Y - Yref, axis=1) / np.maximum(np.linalg.norm(Yref, axis=1), 1e-300)


@pytest.mark.parametrize("wide", [False, True])
def test_four_row_survivors_are_settled_in_the_wave(vc, wide):
    import torch
    from voiceconversion_jl_amd import _lib
    w, mu, sig, X, Yref = _case()
    FT = 2 if wide else 1
    sum_k, base, n4, whitening = _replayed_counts(FT)
    bound = 4 * FT * PER_PAIR * (sum_k + 2)
    allowance = 2 * (4 * FT * PER_PAIR)
    print(f"FT = {FT}: {-(-T // (64 * FT))} workgroups, sum of K_w {sum_k}, bound {bound}; replayed base {base}, four-row survivors {n4}, "
          f"their whitening {whitening}, allowance {allowance}")
    assert whitening > 4 * allowance, (whitening, allowance)         # without a working look the count is base + whitening: it fails below

    g = vc.GMMMap(*julia_model(w, mu, sig))
    xt = torch.from_numpy(np.array(X)).cuda().t()
    _lib.debug_force(_lib.DBG_CONVERT_WIDE_TILES if wide else 0)
    try:
        assert g.convert_plan()[1] == 3
        g.prune_stats(True)
        Y = vc.fvconvert(g, xt).t().cpu().numpy()
        issued = g.convert_plan()[0]
        g.prune_stats(False)
        Y2 = vc.fvconvert(g, xt).t().cpu().numpy()
    finally:
        _lib.debug_force(0)
    err = _frame_err(Y, Yref)
    print(f"FT = {FT}: issued {issued} (bound {bound}, {issued / (4 * FT * PER_PAIR):.1f} workgroup mixtures); "
          f"max per-frame relative error {err.max():.3e}")
    assert issued <= bound, (issued, bound)
    assert issued <= base + allowance, (issued, base, allowance)
    assert np.array_equal(Y, Y2)
    assert np.all(np.isfinite(Y)) and err.max() < TOL, int(np.argmax(err))


@pytest.mark.parametrize("wide", [False, True])
def test_shifted_frames_against_the_dense_loop(vc, wide):
    import torch
    from voiceconversion_jl_amd import _lib
    w, mu, sig, X, _ = _case()
    g = vc.GMMMap(*julia_model(w, mu - 2000.0, sig))
    xt = torch.from_numpy(X - 2000.0).cuda().t()
    force = _lib.DBG_CONVERT_WIDE_TILES if wide else 0
    _lib.debug_force(force | (0 if g.convert_plan()[1] == 3 else _lib.DBG_CONVERT_SHAPE_SCREENED))
    try:
        assert g.convert_plan()[1] == 3
        Y = vc.fvconvert(g, xt).t().clone()
        assert torch.equal(vc.fvconvert(g, xt).t(), Y)
    finally:
        _lib.debug_force(0)
    g.set_prune(float("inf"))
    Yd = vc.fvconvert(g, xt).t().clone()
    rel = float((torch.linalg.norm(Y - Yd, dim=1) / torch.linalg.norm(Yd, dim=1)).max())
    print(f"shifted by -2000, {'two tiles' if wide else 'one tile'} per wave: max per-frame difference from the dense loop {rel:.3e}")
    assert bool(torch.isfinite(Y).all()) and rel < 1e-13
