"""The group radius of the screened fvconvert (csrc/gmmmap_screen.hpp, step 1b; csrc/gmmmap_prepare.cpp: screen_radius_*).

A workgroup all of whose frames have one group key g and lie inside the radius the host certified for g (l_g >= lmin[g]) skips the
screen: steps 2 and 3 could only find out that every other mixture is more than prune under l_g.  It skips a proof, never a term, so
y must be the flag-off run's (`DBG_SCREEN_NO_RADIUS`: every workgroup runs the screen) bit for bit, and WHICH workgroups skip is
replayed here in numpy: the keys (nearest source mean over the first 24 features, stable sort), l_g of every frame and the host's
own lmin (`_lib.screen_radius_host`, checked against numpy by tests/test_screen_radius_host.py).  The skip counter
(`screen_radius_stats()[0]`) must equal the replayed count exactly; the model draws have |z_g|^2 around 40 against radii of 290 and
more, the planted outliers sit 5 % outside, so no frame is near enough to its radius for rounding to decide.

`synth_model(7, 80, M)`, M = 8 and 16, D = 40, the first 8192 + 17 of the 8192 + 127 draws of `sample_frames(13, ...)` (the prefix
the other screen tests use), one tile per wave (64-frame workgroups) and, with `DBG_CONVERT_WIDE_TILES`, two (128).  The handles are
created with four screening rows (`DBG_SCREEN_ROWS4`), so that the bf16 screen runs as on the benchmark's model; one case runs the
FP64 screen (`DBG_SCREEN_FP64`).
"""
import numpy as np
import pytest

from conftest import julia_model

pytestmark = pytest.mark.gpu

D = 40
T = 8192 + 17
KEY_DIMS = 24
TOL = 1e-9


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


_CACHE = {}


def _case(M, lam_lo=1e-5):
    if (M, lam_lo) not in _CACHE:
        import synthdata as sd
        w, mu, sig = sd.synth_model(7, 2 * D, M, lam_lo=lam_lo)
        X = sd.sample_frames(13, w, mu, sig, 8192 + 127, 0, D)[:T].copy()
        X.setflags(write=False)
        _CACHE[(M, lam_lo)] = (w, mu, sig, X)
    return _CACHE[(M, lam_lo)]


def _oracle(M):
    if ("oracle", M) not in _CACHE:
        from oracle import c_oracle as co
        w, mu, sig, X = _case(M)
        _CACHE[("oracle", M)] = co.GMMMap(w, mu, sig).fvconvert_mt(X)[0]
    return _CACHE[("oracle", M)]


def _replay(w, mu, sig, X, lmin, per_wg):
    """(workgroups, one-key workgroups, of those certified, the certified workgroups' indices, perm, keys)"""
    M = len(w)
    mux = mu[:, :D]
    Xk = np.nan_to_num(X[:, :KEY_DIMS])
    d2 = (Xk ** 2).sum(1)[:, None] - 2.0 * Xk @ mux[:, :KEY_DIMS].T + (mux[:, :KEY_DIMS] ** 2).sum(1)[None]
    key = np.argmin(d2, axis=1)
    perm = np.argsort(key, kind="stable")
    ks = key[perm]
    lg = np.empty(len(X))
    for m in range(M):
        sel = key == m
        S = sig[m][:D, :D]
        with np.errstate(divide="ignore"):
            lc = np.log(w[m]) - 0.5 * (D * np.log(2.0 * np.pi) + np.linalg.slogdet(S)[1])
        z = np.linalg.solve(np.linalg.cholesky(S), (X[sel] - mux[m]).T)
        lg[sel] = lc - 0.5 * (z ** 2).sum(0)
    lg = lg[perm]
    nwg = one = 0
    cert = []
    for i, p0 in enumerate(range(0, len(X), per_wg)):
        sl = slice(p0, min(len(X), p0 + per_wg))
        nwg += 1
        if len(np.unique(ks[sl])) == 1:
            one += 1
            if np.all(lg[sl] >= lmin[ks[p0]]):                      # (a NaN fails)
                cert.append(i)
    return nwg, one, len(cert), cert, perm, key


def _run(vc, g, X, force):
    """(y, y again, skipped workgroups) under `force`"""
    import torch
    from voiceconversion_jl_amd import _lib
    xt = torch.from_numpy(np.array(X)).cuda().t()
    _lib.debug_force(force | (0 if g.convert_plan()[1] == 3 else _lib.DBG_CONVERT_SHAPE_SCREENED))
    try:
        assert g.convert_plan()[1] == 3
        g.prune_stats(True)
        Y = vc.fvconvert(g, xt).t().cpu().numpy()
        skipped = g.screen_radius_stats()[0]
        g.prune_stats(False)
        Y2 = vc.fvconvert(g, xt).t().cpu().numpy()
    finally:
        _lib.debug_force(0)
    return Y, Y2, skipped


def _make(vc, w, mu, sig):
    from voiceconversion_jl_amd import _lib
    _lib.debug_force(_lib.DBG_SCREEN_ROWS4)                          # (read when the converter is created)
    try:
        return vc.GMMMap(*julia_model(w, mu, sig))
    finally:
        _lib.debug_force(0)


def _on_off(vc, g, X, base, expect=None):
    """y with the certificate, bit for bit the flag-off run's and its own second call's; returns (y, skipped)"""
    from voiceconversion_jl_amd import _lib
    Y, Y2, skipped = _run(vc, g, X, base)
    Yoff, _, skipped_off = _run(vc, g, X, base | _lib.DBG_SCREEN_NO_RADIUS)
    assert skipped_off == 0
    assert np.array_equal(Y, Yoff, equal_nan=True) and np.array_equal(Y, Y2, equal_nan=True)
    if expect is not None:
        assert skipped == expect, (skipped, expect)
    return Y, skipped


def _frame_err(Y, Yref):
    return np.linalg.norm(Y - Yref, axis=1) / np.maximum(np.linalg.norm(Yref, axis=1), 1e-300)


@pytest.mark.parametrize("M,wide,fp64", [(8, False, False), (8, True, False), (16, False, False), (16, True, False), (16, True, True)])
def test_certified_workgroups_skip_the_screen(vc, M, wide, fp64):
    from voiceconversion_jl_amd import _lib
    w, mu, sig, X = _case(M)
    per_wg = 128 if wide else 64
    base = (_lib.DBG_CONVERT_WIDE_TILES if wide else 0) | (_lib.DBG_SCREEN_FP64 if fp64 else 0)
    lmin = _lib.screen_radius_host(*julia_model(w, mu, sig), prune=46.0)[2]
    nwg, one, ncert, cert, perm, key = _replay(w, mu, sig, X, lmin, per_wg)
    print(f"M = {M}, {per_wg}-frame workgroups: {nwg}, one-key {one} ({one / nwg:.0%}), of those certified {ncert}")
    assert 2 * ncert >= nwg                                          # the test looks at something

    g = _make(vc, w, mu, sig)
    assert g.screen_radius_stats()[1], g.screen_radius_stats()       # the certificate is in use for this model
    Y, skipped = _on_off(vc, g, X, base, ncert)
    err = _frame_err(Y, _oracle(M))
    print(f"skipped {skipped} of {nwg} workgroups; max per-frame relative error against the oracle {err.max():.3e}")
    assert np.all(np.isfinite(Y)) and err.max() < TOL, int(np.argmax(err))

    # planted outliers: one frame of each of five certified workgroups moved along its group's lowest-variance direction to
    # |z_g|^2 = 1.05 R_g (a step of a few hundredths: the key stays) -- exactly those workgroups run the screen again
    R = _lib.screen_radius_host(*julia_model(w, mu, sig), prune=46.0)[1]
    Xo = np.array(X)
    hit = cert[:: max(1, len(cert) // 5)][:5]
    for i in hit:
        t = perm[i * per_wg + 3]
        m = key[t]
        lam, V = np.linalg.eigh(sig[m][:D, :D])
        Xo[t] = mu[m, :D] + np.sqrt(1.05 * R[m] * lam[0]) * V[:, 0]
    nwg2, _, ncert2, cert2, _, key2 = _replay(w, mu, sig, Xo, lmin, per_wg)
    assert np.array_equal(key2, key) and sorted(set(cert) - set(cert2)) == sorted(hit) and ncert2 == ncert - len(hit)
    _on_off(vc, g, Xo, base, ncert2)


@pytest.mark.parametrize("wide", [False, True])
def test_edge_cases_keep_y(vc, wide):
    import torch
    from voiceconversion_jl_amd import _lib
    M = 16
    w, mu, sig, X = _case(M)
    per_wg = 128 if wide else 64
    base = _lib.DBG_CONVERT_WIDE_TILES if wide else 0
    lmin = _lib.screen_radius_host(*julia_model(w, mu, sig), prune=46.0)[2]
    ncert = _replay(w, mu, sig, X, lmin, per_wg)[2]
    g = _make(vc, w, mu, sig)

    # a frame of NaN: its workgroup is not certified, whatever group its key put it in (which the replay does not know)
    Xn = np.array(X)
    Xn[4321] = np.nan
    _, skipped = _on_off(vc, g, Xn, base)
    assert 0 < skipped <= ncert + 1, (skipped, ncert)
    # the partly filled last tile (T = 8192 + 17 has one; here a call that ends one frame into a workgroup)
    Tp = 8192 + 1
    _on_off(vc, g, X[:Tp], base, _replay(w, mu, sig, X[:Tp], lmin, per_wg)[2])

    # prune changed to 200 after creation.  The radii shrink (247 -> 150 at the least) but the draws stay inside (|z_g|^2 < 90), so
    # on them alone the count would not move: one frame of each of five certified workgroups is planted BETWEEN the two radii of
    # its group, along the lowest-variance direction -- certified at 46, not at 200, the replayed workgroups exactly; y the dense
    # loop's
    R46, R200, lmin200 = (_lib.screen_radius_host(*julia_model(w, mu, sig), prune=p)[i] for p, i in ((46.0, 1), (200.0, 1), (200.0, 2)))
    assert np.all(R200 < R46) and np.all(R200 > 0.0)
    _, _, _, cert, perm, key = _replay(w, mu, sig, X, lmin, per_wg)
    Xp = np.array(X)
    hit = cert[1:: max(1, len(cert) // 5)][:5]
    for i in hit:
        t = perm[i * per_wg + 5]
        m = key[t]
        lam, V = np.linalg.eigh(sig[m][:D, :D])
        Xp[t] = mu[m, :D] + np.sqrt(0.5 * (R46[m] + R200[m]) * lam[0]) * V[:, 0]
    _, _, ncert46, cert46, _, keyp = _replay(w, mu, sig, Xp, lmin, per_wg)
    _, _, ncert200, cert200, _, _ = _replay(w, mu, sig, Xp, lmin200, per_wg)
    print(f"{per_wg}-frame workgroups certified: {ncert46} at prune 46, {ncert200} at 200")
    assert np.array_equal(keyp, key) and ncert46 == ncert and sorted(set(cert46) - set(cert200)) == sorted(hit)
    assert ncert200 < ncert46
    _on_off(vc, g, Xp, base, ncert46)
    g.set_prune(200.0)
    Y200, _ = _on_off(vc, g, Xp, base, ncert200)
    g.set_prune(float("inf"))
    Yd = vc.fvconvert(g, torch.from_numpy(Xp).cuda().t()).t().cpu().numpy()
    assert _frame_err(Y200, Yd).max() < 1e-13
    g.set_prune(46.0)
    _on_off(vc, g, X, base, ncert)                                   # and back

    # a zero-weight mixture that is some frames' nearest mean: its groups are never certified
    w0 = w.copy()
    k = int(np.argmax(w))
    w0[k] = 0.0
    w0 /= w0.sum()
    lmin0 = _lib.screen_radius_host(*julia_model(w0, mu, sig), prune=46.0)[2]
    assert lmin0[k] == np.inf
    _, _, ncert0, _, _, key0 = _replay(w0, mu, sig, X, lmin0, per_wg)
    assert (key0 == k).sum() > per_wg and 0 < ncert0 < ncert
    _on_off(vc, _make(vc, w0, mu, sig), X, base, ncert0)

    # the model and the frames shifted by -2000: y stays the flag-off run's.  No count: the bf16 grouping keys of such frames
    # (-2 mu'x of the order 1e8 against differences of tens) are not the nearest means, so hardly a workgroup has one key
    gs = _make(vc, w, mu - 2000.0, sig)
    assert gs.screen_radius_stats()[1]
    _, skipped = _on_off(vc, gs, X - 2000.0, base)
    print(f"shifted by -2000: {skipped} workgroups skipped the screen")

    # lam_lo = 1e-2 forced to shape 3: few frames lie inside a radius -- whether the handle takes the test at all is the library's
    # decision (screen_radius_stats()[1]); where it does, the count is the replayed one, where it does not, zero
    wb, mub, sigb, Xb = _case(M, lam_lo=1e-2)
    gb = _make(vc, wb, mub, sigb)
    lminb = _lib.screen_radius_host(*julia_model(wb, mub, sigb), prune=46.0)[2]
    ncertb = _replay(wb, mub, sigb, Xb, lminb, per_wg)[2]
    _, on, frac = gb.screen_radius_stats()
    print(f"lam_lo = 1e-2: share of the profile frames inside {frac:.3f}, in use {on}, replayed certified workgroups {ncertb}")
    assert ncertb < ncert
    _on_off(vc, gb, Xb, base, ncertb if on else 0)
