"""GPU: GMMMap fvconvert / predict_proba / predict on frames whose posterior is SHARED among the mixtures, on every kernel
path, against the longdouble restatement tests/gmmmap_restatement.py and inside the bounds derived there (the tests of
tests/test_gpu_gmmmap.py draw from models whose frames have one live mixture each outside D = 40: every posterior is 0 or 1).

  tied_model (both settings)   y inside convert_bound element by element; |P / P* - 1| inside posterior_bound for every
                               P* >= 1e-300; predict = the restatement's index wherever its margin exceeds 2 max_m B_tm
  source_tied_ladder           the posterior of every frame is the weight vector (0.73 ... 7e-305): P against the weights
                               themselves; y against sum_m w_m e_m; two equal weights: predict returns the smaller index

Paths: the generic kernel; the tile kernel with one tile per wave (dense, broad, peaked) and two (DBG_CONVERT_WIDE_TILES); the
eight-wave tile kernel either side of DP = 72; logdens_tiled_kernel + convert_from_logdens_kernel (one and two 64-mixture
groups); grouped calls with the library's plan and the screen forced; tile MODE 1 / logdens_tiled_kernel / generic MODE 1 +
posterior_finish_kernel in its five lanes-per-frame layouts; predict with the early exit, without it, in two passes, screened.

Measured on an MI355X (the module prints all of it: -s).  Per path family: the largest error / bound, and the largest bound
itself -- y relative to the frame's largest |y|, posteriors relative, in eps = 2^-53.  The bounds are worst-case ones: the
conditioning terms of B (Cholesky, triangular inverse) are a thousand times its |z|^2 / 2 term and grow with D, so above D = 80
the y bound is wider than the frame-relative 1e-9 of tests/test_gpu_gmmmap.py, which stays in force beside it.  What the
bounds buy is that they are RELATIVE (a posterior of 7e-305 is held like one of 0.7) and stated on frames where every part
of the softmax works.
                                              error / bound    bound
    fvconvert, tied: generic kernel           8.9e-5           6.6e-10 of max |y|
      tile kernel, one or two tiles per wave  2.0e-4           1.6e-9       (dense = broad = peaked)
      eight-wave tile kernel                  2.6e-6           4.9e-9
      above 80, streamed tiles + softmax      8.9e-7           3.0e-8
      above 80, generic kernel                9.1e-7           3.0e-8
      grouped, own plan / screened / FP64     2.2e-5           1.6e-9
    fvconvert, ladders: generic               5.0e-4           5.2e-12
      tile kernels                            2.3e-5           3.0e-10
      above 80                                3.6e-6           1.5e-9
    predict_proba, tied: generic MODE 1       1.6e-2           4.2e4 eps
      tile MODE 1                             4.1e-4           2.4e7 eps
      logdens_tiled_kernel                    6.7e-5           2.7e8 eps (D = 160)
    predict_proba, ladders: generic MODE 1    6.7e-2           2.1e4 eps
      tile MODE 1                             1.6e-3           4.9e6 eps
      logdens_tiled_kernel                    8.8e-5           4.5e7 eps (D = 160)
    rows sum to 1                             within 0.12 (M + 16) eps on every path.  With posterior_finish_kernel's earlier form
                                              exp(l - (u + log s)) the ladders at D = 100 and 160, M = 8 missed it 2.4 times over
                                              (58 eps: the rounding of lse puts |lse| eps on every posterior of a frame); the
                                              kernel now evaluates exp(l - u) / s.
    predict                                   0.00 % of the frames left out (cap 1 %) on every path

Not checked: the tied-model posterior cases with D = 160 and M = 64, 65, 130 compare 43 of their 131 frames with the
longdouble reference (rs.posterior_checked_frames; the others are held to finite values and rows that sum to 1).  No counter of
the library tells logdens_tiled_kernel + the softmax kernel from the generic kernel, or the screened arg-max from the
early-exit one: those legs rely on the dispatch rules (D, set_kernel, the debug flag).
"""
import contextlib
import functools

import numpy as np
import pytest

from conftest import julia_model
import gmmmap_restatement as rs

pytestmark = pytest.mark.gpu
RECORD = {}            # path family -> largest error / bound seen
HELD = {}              # path family -> the largest bound itself: posteriors in eps (relative), y relative to the frame's largest |y|
LEFT_OUT = {}          # path family -> largest share of frames predict was not held to a single index on


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    yield m
    for k in sorted(RECORD):
        print(f"\n[shared posteriors] {k}: largest error / bound {RECORD[k]:.4g}", end="")
    for k in sorted(HELD):
        print(f"\n[shared posteriors] {k}: largest bound {HELD[k]:.3g}", end="")
    for k in sorted(LEFT_OUT):
        print(f"\n[shared posteriors] {k}: predict left out {100 * LEFT_OUT[k]:.2f} % of the frames", end="")
    print()


def note(family, ratio):
    RECORD[family] = max(RECORD.get(family, 0.0), float(ratio))
    return float(ratio)


@contextlib.contextmanager
def forced(flags):
    from voiceconversion_jl_amd import _lib
    _lib.debug_force(flags)
    try:
        yield
    finally:
        _lib.debug_force(0)


def dev(X, pad=0):
    """(T,D) numpy -> (D,T) device tensor with unit stride along D and a leading dimension of D + pad"""
    import torch
    T, D = X.shape
    buf = torch.full((T, D + pad), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :D] = torch.from_numpy(np.array(X, order="C")).cuda()
    return buf[:, :D].t()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def tied_case(D, M, T, setting, zero=-1, posterior=False):
    """model, its own frames and the restatement's results and bounds; made once, never written to.  sel: the frames the
    reference covers -- all of them but for the posterior cases with D = 160, M >= 64 (rs.posterior_checked_frames)"""
    w, mu, sig = rs.tied_model(100 + D + M, 2 * D, M, **rs.SETTINGS[setting])
    if zero >= 0:
        w = w.copy()
        w[zero] = 0.0
        w /= w.sum()
    X = rs.frames(200 + D, w, mu, sig, T)
    sel = rs.posterior_checked_frames(D, M, T) if posterior else np.arange(T)
    Xs = X[sel]
    mdl = rs.Model(w, mu, sig)
    if posterior:
        L = mdl.logdens(Xs)
        P = rs.posterior(L)
        out = dict(w=w, mu=mu, sig=sig, X=X, sel=sel, P=P, L=L, B=mdl.logdens_bound(Xs), R=mdl.posterior_bound(Xs, P)[0])
    else:
        Y, P, L = mdl.convert(Xs)
        out = dict(w=w, mu=mu, sig=sig, X=X, sel=sel, Y=Y, P=P, YB=mdl.convert_bound(Xs), YBdense=mdl.convert_bound(Xs, np.inf))
    for a in out.values():
        a.setflags(write=False)
    return out


def check_y(family, Y, c, dense=False):
    """Y (D,T) from the device against the restatement, element by element inside the bound"""
    Y = np.asarray(Y).T
    assert Y.shape == c["X"].shape and np.all(np.isfinite(Y))
    YB = c["YBdense"] if dense else c["YB"]
    f = np.abs(Y - c["Y"]) / YB
    HELD["y / max |y|, " + family] = max(HELD.get("y / max |y|, " + family, 0.0), float(np.max(YB / np.abs(np.asarray(c["Y"], dtype=np.float64)).max(axis=1, keepdims=True))))
    r = note(family, f.max())
    assert np.all(f <= 1.0), (family, r)
    return r


def check_p(family, P, Pref, R):
    """P (M,T) from the device: |P / P* - 1| inside R wherever P* >= 1e-300, exactly 0 where P* is; rows sum to 1"""
    P = np.asarray(P).T
    M = P.shape[1]
    held = np.asarray(Pref, dtype=np.float64) >= 1e-300
    HELD["P relative, in eps, " + family] = max(HELD.get("P relative, in eps, " + family, 0.0), float(np.max(np.broadcast_to(R, P.shape)[held]) / rs.EPS))
    zero = np.asarray(Pref) == 0
    assert np.all(P[zero] == 0.0) and np.all(np.isfinite(P))
    f = np.abs(np.log(P[held].astype(rs.LD) / np.broadcast_to(Pref, P.shape)[held])) / np.broadcast_to(R, P.shape)[held]
    r = note(family, f.max())
    assert np.all(f <= 1.0), (family, r)
    rows = np.abs(P.astype(rs.LD).sum(axis=1) - 1) / ((M + 16) * rs.EPS)
    note(family + ", row sums / ((M + 16) eps)", rows.max())
    assert np.all(rows <= 1.0), (family, float(rows.max()))
    return r


def check_predict(family, idx, c):
    """equal to the restatement's first maximum where its margin exceeds 2 max_m B_tm, one of the mixtures within that margin
    of the maximum otherwise; at most 1 % of the frames are of the second kind"""
    idx = np.asarray(idx)[c["sel"]]
    L = np.asarray(c["L"], dtype=np.float64)
    margin = 2 * np.where(np.isfinite(c["B"]), c["B"], 0.0).max(axis=1)
    Ls = np.sort(L, axis=1)
    clear = Ls[:, -1] - Ls[:, -2] > margin
    LEFT_OUT[family] = max(LEFT_OUT.get(family, 0.0), float(1 - clear.mean()))
    assert 1 - clear.mean() <= 0.01, (family, float(1 - clear.mean()))
    assert np.array_equal(idx[clear], rs.predict(c["L"])[clear])
    assert np.all(L[np.arange(len(idx)), idx - 1] >= Ls[:, -1] - margin)


# ------------------------------------------------------------------------------------------- fvconvert on tied models
@pytest.mark.parametrize("setting", list(rs.SETTINGS))
@pytest.mark.parametrize("D,M,T,kernel", [s + (0,) for s in rs.GENERIC_SHAPES] + [(40, 9, 131, 1)])
def test_generic_kernel_converts_shared_frames(vc, D, M, T, kernel, setting):
    c = tied_case(D, M, T, setting)
    g = vc.GMMMap(*julia_model(c["w"], c["mu"], c["sig"]))
    g.set_kernel(kernel)
    assert g.convert_plan()[1] == -1                                   # no tile kernel: gmmmap_generic_kernel
    XT = np.asfortranarray(c["X"].T)
    r = check_y("generic kernel", vc.fvconvert(g, XT), c)               # host pointers
    check_y("generic kernel", host(vc.fvconvert(g, dev(c["X"], pad=3))), c)
    print(f"generic D={D} M={M} {setting}: {r:.3g} of the bound")


def _loop_shapes(vc, g, c, family, wide):
    """dense, broad and peaked loops of the tile kernel on one case (device tensors), optionally two tiles per wave"""
    from voiceconversion_jl_amd import _lib
    Xd = dev(c["X"])
    w = _lib.DBG_CONVERT_WIDE_TILES if wide else 0
    out = []
    g.set_prune(float("inf"))
    with forced(w):
        assert g.convert_plan()[1] == 0
        out.append(check_y(family + ", dense", host(vc.fvconvert(g, Xd)), c, dense=True))
    g.set_prune(rs.PRUNE)
    for shape, flag in ((1, _lib.DBG_CONVERT_SHAPE_BROAD), (2, _lib.DBG_CONVERT_SHAPE_PEAKED)):
        with forced(flag | w):
            assert g.convert_plan()[1] == shape
            out.append(check_y(family + (", broad" if shape == 1 else ", peaked"), host(vc.fvconvert(g, Xd)), c))
    return out


@pytest.mark.parametrize("setting", list(rs.SETTINGS))
@pytest.mark.parametrize("D,M,T", rs.TILE_SHAPES)
def test_tile_kernel_converts_shared_frames(vc, D, M, T, setting):
    c = tied_case(D, M, T, setting)
    g = vc.GMMMap(*julia_model(c["w"], c["mu"], c["sig"]))
    r = _loop_shapes(vc, g, c, "tile kernel, one tile per wave", False)
    if D in rs.WIDE_TILE_DIMS:
        r += _loop_shapes(vc, g, c, "tile kernel, two tiles per wave", True)
    if (D, M) == (25, 9):                                               # the host-pointer entry and a leading dimension > D
        check_y("tile kernel, one tile per wave, entries", vc.fvconvert(g, np.asfortranarray(c["X"].T)), c)
        check_y("tile kernel, one tile per wave, entries", host(vc.fvconvert(g, dev(c["X"], pad=5))), c)
    print(f"tile D={D} M={M} {setting}: {max(r):.3g} of the bound")


@pytest.mark.parametrize("setting", list(rs.SETTINGS))
@pytest.mark.parametrize("D,M,T", rs.EIGHT_WAVE_SHAPES)
def test_eight_wave_kernel_converts_shared_frames(vc, D, M, T, setting):
    c = tied_case(D, M, T, setting)
    g = vc.GMMMap(*julia_model(c["w"], c["mu"], c["sig"]))
    r = _loop_shapes(vc, g, c, "eight-wave tile kernel", False)
    if (D, M) == (57, 6):
        check_y("eight-wave tile kernel, entries", vc.fvconvert(g, np.asfortranarray(c["X"].T)), c)
        check_y("eight-wave tile kernel, entries", host(vc.fvconvert(g, dev(c["X"], pad=1))), c)
    print(f"eight waves D={D} M={M} {setting}: {max(r):.3g} of the bound")


@pytest.mark.parametrize("setting", list(rs.SETTINGS))
@pytest.mark.parametrize("D,M,T", rs.FALLBACK_SHAPES)
def test_fallback_above_80_converts_shared_frames(vc, D, M, T, setting):
    """logdens_tiled_kernel + convert_from_logdens_kernel, one mixture without weight, pruning on and off, and the generic
    kernel on the same frames"""
    c = tied_case(D, M, T, setting, zero=2)
    g = vc.GMMMap(*julia_model(c["w"], c["mu"], c["sig"]))
    Xd = dev(c["X"])
    # no tile kernel and none of its counters: with kernel 0 the dispatch leaves logdens_tiled_kernel + the softmax kernel (16 < D
    # <= 160), with kernel 1 the generic one; the library has no counter that tells those two apart
    assert g.convert_plan()[1] == -1
    g.prune_stats(True)
    r = [check_y("above 80: streamed tiles + softmax kernel", host(vc.fvconvert(g, Xd)), c)]
    assert g.prune_stats(False) == 0
    g.set_prune(float("inf"))
    r.append(check_y("above 80: streamed tiles + softmax kernel, dense", host(vc.fvconvert(g, Xd)), c, dense=True))
    g.set_prune(rs.PRUNE)
    g.set_kernel(1)
    r.append(check_y("above 80: generic kernel", host(vc.fvconvert(g, Xd)), c, dense=True))
    g.set_kernel(0)
    if D == 100:
        check_y("above 80: entries", vc.fvconvert(g, np.asfortranarray(c["X"].T)), c)
        check_y("above 80: entries", host(vc.fvconvert(g, dev(c["X"], pad=7))), c)
    print(f"above 80 D={D} M={M} {setting}: {max(r):.3g} of the bound")


@pytest.mark.parametrize("setting", list(rs.SETTINGS))
@pytest.mark.parametrize("D,M,T", rs.GROUPED_SHAPES)
def test_grouped_calls_convert_shared_frames(vc, D, M, T, setting):
    """the grouping threshold: frames sorted by nearest source mean, the library's own plan and the screen forced -- on a tied
    model every mixture survives the screen"""
    from voiceconversion_jl_amd import _lib
    c = tied_case(D, M, T, setting)
    g = vc.GMMMap(*julia_model(c["w"], c["mu"], c["sig"]))
    Xd = dev(c["X"])
    g.prune_stats(True)
    r = [check_y("grouped call, the library's plan", host(vc.fvconvert(g, Xd)), c)]
    issued, shape, _, _ = g.convert_plan()
    assert shape in (1, 2, 3) and issued > 0 and g.prune_stats(False) > 0          # a tile or screen kernel ran and counted
    with forced(_lib.DBG_CONVERT_SHAPE_SCREENED):
        assert g.convert_plan()[1] == 3
        r.append(check_y("grouped call, screened", host(vc.fvconvert(g, Xd)), c))
        r.append(check_y("grouped call, screened", vc.fvconvert(g, np.asfortranarray(c["X"].T)), c))
    with forced(_lib.DBG_CONVERT_SHAPE_SCREENED | _lib.DBG_SCREEN_FP64):
        r.append(check_y("grouped call, screened in FP64", host(vc.fvconvert(g, dev(c["X"], pad=2))), c))
    print(f"grouped D={D} M={M} {setting}: {max(r):.3g} of the bound")


# ------------------------------------------------------------------------------------ predict_proba, relative; predict
def _logdens_family(D):
    return "generic MODE 1" if D <= 12 else ("tile MODE 1" if D <= 80 else "logdens_tiled_kernel")


@pytest.mark.parametrize("D,M", rs.POSTERIOR_TIED_SHAPES)
def test_posteriors_of_shared_frames_are_relative(vc, D, M):
    from voiceconversion_jl_amd import _lib
    c = tied_case(D, M, 131, "default", posterior=True)
    sel = c["sel"]                                                      # all 131 frames but for D = 160, M >= 64: the first 13, then every fourth
    assert np.array_equal(sel[:13], np.arange(13))
    g = vc.GMMMap(*julia_model(c["w"], c["mu"], c["sig"]))
    fam = f"posterior, tied model, {_logdens_family(D)}"
    P13 = vc.predict_proba(g.px, np.asfortranarray(c["X"][:13].T))      # the last wave holds dead frame slots
    r = [check_p(fam, P13, c["P"][:13], c["R"][:13])]
    P = vc.predict_proba(g.px, np.asfortranarray(c["X"].T))
    assert np.all(np.isfinite(P)) and np.all(np.abs(P.sum(axis=0) - 1) <= (M + 16) * rs.EPS)          # every frame
    r.append(check_p(fam, P[:, sel], c["P"], c["R"]))
    r.append(check_p(fam, host(vc.predict_proba(g.px, dev(c["X"], pad=3)))[:, sel], c["P"], c["R"]))
    XT = np.asfortranarray(c["X"].T)
    check_predict(f"predict, tied model, {_logdens_family(D)}", vc.predict(g.px, XT), c)
    for flag in (_lib.DBG_PREDICT_NO_EARLY_EXIT, _lib.DBG_PREDICT_TWO_PASS):
        with forced(flag):
            check_predict(f"predict, tied model, {_logdens_family(D)}", vc.predict(g.px, XT), c)
    print(f"posterior tied D={D} M={M}: {max(r):.3g} of the bound")


@functools.lru_cache(maxsize=None)
def ladder_case(D, gaps, T):
    """a source-tied ladder, its frames, the weights as every frame's posterior, y = sum w e, and the bounds"""
    w, mu, sig = rs.source_tied_ladder(500 + D, D, gaps)
    X = rs.frames(600 + D, w, mu, sig, T)
    mdl = rs.Model(w, mu, sig)
    Pw = np.broadcast_to(rs.ladder_posterior(w), (T, len(w)))
    R, _ = mdl.posterior_bound(X, Pw)
    out = dict(w=w, mu=mu, sig=sig, X=X, P=Pw, R=R, mdl=mdl)
    for k in ("w", "mu", "sig", "X", "R"):
        out[k].setflags(write=False)
    return out


@pytest.mark.parametrize("M", rs.POSTERIOR_MS)
@pytest.mark.parametrize("D", rs.POSTERIOR_DIMS)
def test_ladder_posteriors_are_the_weights(vc, D, M):
    """P against the weights themselves, relative: entries of 1.5e-9, 2e-20, 3.8e-131 and 7e-305 (divided by the repeats of the
    ladder) are held like the largest; M either side of every boundary between posterior_finish_kernel's five layouts"""
    c = ladder_case(D, rs.ladder_gaps(M), 131)
    g = vc.GMMMap(*julia_model(c["w"], c["mu"], c["sig"]))
    fam = f"posterior, ladder, {_logdens_family(D)}"
    r = []
    for T in (13, 131):
        P = vc.predict_proba(g.px, np.asfortranarray(c["X"][:T].T))
        assert np.all(P > 0) and P.min() < 1e-300                     # the 700-nat step is there and not flushed to zero
        r.append(check_p(fam, P, c["P"][:T], c["R"][:T]))
    print(f"posterior ladder D={D} M={M}: {max(r):.3g} of the bound (relative bounds {c['R'].min():.2e} ... {c['R'].max():.2e})")


@pytest.mark.parametrize("D", [7, 40, 56, 100])
def test_equal_weights_on_the_ladder_go_to_the_smaller_index(vc, D):
    """mixtures 2 and 4 tie bit for bit on every frame: predict returns 2 whatever order the kernel visits the mixtures in"""
    from voiceconversion_jl_amd import _lib
    T = 8192 + 7 if D in (40, 56) else 131
    c = ladder_case(D, rs.LADDER_TIED, T)
    g = vc.GMMMap(*julia_model(c["w"], c["mu"], c["sig"]))
    XT = np.asfortranarray(c["X"].T)
    small = np.asfortranarray(c["X"][:131].T)
    assert np.all(vc.predict(g.px, small) == 2)                        # early exit (tile dimensions) / two passes (the others)
    for flag in (_lib.DBG_PREDICT_NO_EARLY_EXIT, _lib.DBG_PREDICT_TWO_PASS, _lib.DBG_PREDICT_NO_SCREEN):
        with forced(flag):
            assert np.all(vc.predict(g.px, small) == 2), flag
    assert np.all(host(vc.predict(g.px, dev(c["X"][:131], pad=2))) == 2)
    if T > 8192:
        with forced(_lib.DBG_PREDICT_SCREEN):
            assert np.all(vc.predict(g.px, XT) == 2)
            assert np.all(host(vc.predict(g.px, dev(c["X"]))) == 2)
        assert np.all(vc.predict(g.px, XT) == 2)                        # the library's own choice at this length
    P = vc.predict_proba(g.px, small)
    assert np.array_equal(P[1], P[3])


# ------------------------------------------------------------------------------------------------ fvconvert on the ladders
@pytest.mark.parametrize("order", list(rs.LADDER_ORDERS))
@pytest.mark.parametrize("D", [7, 40, 56, 100])
def test_ladder_conversion_against_the_weighted_sum(vc, D, order):
    """y against sum_m w_m e_m(x) in longdouble (no exponential in the reference), with the largest weight first, in the middle
    and last: every order in which the running maximum of the online softmax can be overtaken"""
    from voiceconversion_jl_amd import _lib
    c = ladder_case(D, rs.LADDER_ORDERS[order], 197)
    mdl = c["mdl"]
    ref = dict(X=c["X"], Y=rs.ladder_convert(c["X"], c["w"], c["mu"], c["sig"]), YB=mdl.convert_bound(c["X"]), YBdense=mdl.convert_bound(c["X"], np.inf))
    g = vc.GMMMap(*julia_model(c["w"], c["mu"], c["sig"]))
    fam = f"ladder conversion, {'generic kernel' if D <= 16 else ('tile kernels' if D <= 80 else 'above 80')}"
    Xd = dev(c["X"])
    r = [check_y(fam, host(vc.fvconvert(g, Xd)), ref), check_y(fam, vc.fvconvert(g, np.asfortranarray(c["X"].T)), ref)]
    if 16 < D <= 80:
        for flag in (_lib.DBG_CONVERT_SHAPE_BROAD, _lib.DBG_CONVERT_SHAPE_PEAKED, _lib.DBG_CONVERT_SHAPE_BROAD | _lib.DBG_CONVERT_WIDE_TILES):
            with forced(flag):
                r.append(check_y(fam, host(vc.fvconvert(g, Xd)), ref))
    g.set_prune(float("inf"))
    r.append(check_y(fam, host(vc.fvconvert(g, Xd)), ref, dense=True))
    print(f"ladder conversion D={D} largest weight {order}: {max(r):.3g} of the bound")
