"""GPU: the default trajectory conversion (TrajectoryGMMMap with full conditional precisions: traj_g_mfma_kernel / traj_g_kernel,
traj_solve_blk_kernel<D> + traj_backsub_blk_kernel<D>, traj_solve_kernel, traj_solve_big_kernel<PK>) against the long-double
reference of tests/traj_full_restatement.py, at every solver instantiation, every short length and with mixture sequences that
push the grouping.

Tolerance: relerr(y, ref) < 64 cond 2^-53 PER UTTERANCE (relerr is max-abs over max-abs: every frame is held), cond the
condition number of that utterance's P as the reference reports it -- cond_2 of P, or above D T = 4000 an upper bound of it.
tests/test_traj_full_restatement_host.py ties the bar to plain FP64: numpy's sparse LU attains an eighth of it.  The bar holds
for every path alike; no path needs a constant of its own (measured: profiles/traj_full_parity/README.md).  The inputs
prescribe the mixture sequence with >= 10 nats to the runner-up (asserted), so the device's arg-max is asserted too.

Every utterance prints  path D T cond err err/(cond 2^-53)  (pytest -s)."""
import functools

import numpy as np
import pytest

import traj_full_restatement as R
from conftest import julia_model, relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def _conv(vc, mdl, T):
    g = vc.GMMMap(*julia_model(*mdl))
    return g, vc.TrajectoryGMMMap(g, T)


def _check(y, ref, path, D):
    """y (D,T) of the device against (y (T,D), gap, cond, mhat) of the reference"""
    yref, gap, cond, _ = ref
    T = yref.shape[0]
    assert y.shape == (D, T)
    if T == 0:
        return
    assert gap >= R.MIN_GAP, (D, T, gap)
    err = relerr(y, yref.T)
    print(f"PARITY {path} D={D} T={T} cond={cond:.4g} err={err:.3e} ratio={err / (cond * R.EPS):.2f}")
    assert err < R.tolerance(cond), (path, D, T, err, R.tolerance(cond))


@functools.lru_cache(maxsize=None)
def _short(D):
    """the batch of (a): T = 1..13, 16, 17, 33 and an empty utterance in the middle -> (model, [X (2D,T)], [s], [reference]);
    made once (the references are R.case's, cached there), never written to"""
    M, kind = R.SHORT[D]
    mdl, _, Xs, ss, refs = R.case(D, M, kind, R.SHORT_TS)
    empty = (np.zeros((0, D), dtype=R.LD), np.inf, 1.0, np.zeros(0, dtype=np.int64))
    k = 5
    batch = [np.asfortranarray(X.T) for X in Xs]
    return (mdl, batch[:k] + [np.zeros((2 * D, 0), order="F")] + batch[k:], ss[:k] + [np.zeros(0, dtype=np.int64)] + ss[k:],
            refs[:k] + [empty] + refs[k:])


def _check_batch(vc, g, Ys, batch, ss, refs, path, D):
    assert len(Ys) == len(batch)
    for y, X, s, ref in zip(Ys, batch, ss, refs):
        _check(y, ref, path, D)
        if X.shape[1]:
            assert np.array_equal(vc.predict(g.px, X), s), (path, D, X.shape[1])


# ----------------------------------------------------------------- a. every solver instantiation, every short length
@pytest.mark.parametrize("D", [12, 16, 20, 24, 25, 30, 32, 40, 46,          # blocked instantiations
                               13, 35, 41,                                  # padded into 16, 40, 46
                               47, 64,                                      # big solver, window packed in LDS
                               65, 72])                                     # big solver, window in HBM
def test_every_instantiation_every_short_length(vc, D):
    """T = 1..5: the stencil without neighbours; RING - 1, RING, RING + 1 of the back substitution's 3 (D = 46) and 5 (D = 32,
    40) panel slots; 8, 9, 16, 17: the factorisation's flush every eight steps, one step deferred; 33.  M = 32 with `cycle` at
    D = 12 and 24: every used mixture has one frame, so every 16-frame tile has a single live slot, the padded slots exceed T
    many times (the 16 M idx slack of gperm), and `last` (D = 25, 35, 72) leaves every mixture in front of the used one empty."""
    mdl, batch, ss, refs = _short(D)
    g, t = _conv(vc, mdl, 33)
    Ys = t.fvconvert_batch(batch)
    _check_batch(vc, g, Ys, batch, ss, refs, "default", D)
    for X, y in zip(batch, Ys):                       # batch == single call, bit for bit
        if X.shape[1] in (1, 5, 33):
            assert np.array_equal(vc.fvconvert(t, X), y), (D, X.shape[1])


# ----------------------------------------------------------------- b. the partner paths against the same reference
@pytest.mark.parametrize("D,flags", [(12, ("GENERIC",)), (32, ("GENERIC",)), (46, ("GENERIC",)),
                                     (12, ("G_SCALAR",)), (32, ("G_SCALAR",)), (46, ("G_SCALAR",)),
                                     (12, ("GENERIC", "G_SCALAR"))])
def test_partner_paths_against_the_reference(vc, D, flags):
    """the runtime-D LDS-window solver (traj_solve_kernel) and the one-workgroup-per-frame g_t kernel (traj_g_kernel), which the
    other tests only compare with the default path"""
    from voiceconversion_jl_amd import _lib
    mdl, batch, ss, refs = _short(D)
    g, t = _conv(vc, mdl, 33)
    mask = 0
    for f in flags:
        mask |= getattr(_lib, "DBG_TRAJ_" + f)
    _lib.debug_force(mask)
    try:
        Ys = t.fvconvert_batch(batch)
    finally:
        _lib.debug_force(0)
    _check_batch(vc, g, Ys, batch, ss, refs, "+".join(flags), D)


# ----------------------------------------------------------------- c. chunk edges of the grouping
@pytest.mark.parametrize("D,M,kind,Ts", [(12, 32, "runs", (127, 128, 129, 257)), (12, 32, "rand", (127, 128, 129, 257)),
                                         (24, 9, "rand", (193,)), (40, 8, "runs", (321,))])
def test_chunk_edges_of_the_grouping(vc, D, M, kind, Ts):
    """the counting sort takes 64 NT frames at a time (NT row tiles of 2D: 128 frames at D = 12, 192 at 24, 320 at 40): one
    frame short of a chunk, a full chunk, one frame into the second, two chunks and one, with up to 32 mixtures in a chunk and
    runs of 15, 16, 17, 1, 31, 32, 33 frames against the 16-frame tiles.  D T > 4000 (D = 24, 40): the cond upper bound."""
    mdl, _, Xs, ss, refs = R.case(D, M, kind, Ts)
    g, t = _conv(vc, mdl, max(Ts))
    batch = [np.asfortranarray(X.T) for X in Xs]
    Ys = t.fvconvert_batch(batch)
    _check_batch(vc, g, Ys, batch, ss, refs, "default", D)


# ----------------------------------------------------------------- d. workgroups per utterance
@pytest.mark.parametrize("D", [12, 40])
def test_workgroups_per_utterance_leave_the_bits_alone(vc, D):
    """`split`, the workgroups of traj_g_mfma_kernel that share an utterance, is the largest power of two <= 8 with
    2 n split <= CUs (traj_run): on 256 CUs the 17 utterances of (a) run with 8, their 16 non-empty ones repeated 3, 5 and 9
    times (n = 48, 80, 144) with 4, 2 and 1.  The grouped order is a function of the data alone, so every copy equals the
    original batch's result bit for bit."""
    mdl, batch, ss, refs = _short(D)
    g, t = _conv(vc, mdl, 33)
    Y0 = t.fvconvert_batch(batch)
    _check_batch(vc, g, Y0, batch, ss, refs, "default", D)
    live = [(X, y) for X, y in zip(batch, Y0) if X.shape[1]]
    assert len(live) == 16
    for rep in (3, 5, 9):
        Ys = t.fvconvert_batch([X for X, _ in live] * rep)
        assert len(Ys) == 16 * rep
        for i, y in enumerate(Ys):
            assert np.array_equal(y, live[i % 16][1]), (D, rep, i)


# ----------------------------------------------------------------- e. ill-conditioned P
@pytest.mark.parametrize("D,M,kind,T", [(12, 4, "rand", 50), (32, 4, "runs", 33)])
def test_ill_conditioned_normal_matrix(vc, D, M, kind, T):
    """delta rows and columns of every Sigma scaled by 1e-2: cond_2(P) in the thousands (D = 32: the eight-wave variant of the
    blocked solver), same bar"""
    mdl, _, Xs, ss, refs = R.case(D, M, kind, (T,), True)
    cond = refs[0][2]
    assert cond > 1e3 and R.tolerance(cond) < 1e-9, cond           # harder than the other cases, and not vacuous
    g, t = _conv(vc, mdl, T)
    X = np.asfortranarray(Xs[0].T)
    _check_batch(vc, g, [vc.fvconvert(t, X)], [X], ss, refs, "default-ill", D)


# ----------------------------------------------------------------- f. vc chunking
def test_vc_chunks_against_the_reference_of_each_chunk(vc):
    """T = 33 in chunks of length(c) = 13: 13, 13 and 7 frames, each an utterance of its own; the power row is copied through"""
    import torch
    D, L = 12, 13
    M, kind = R.SHORT[D]
    mdl, ft, Xs, _, _ = R.case(D, M, kind, R.SHORT_TS)
    X = Xs[-1]
    T = X.shape[0]
    assert T == 33
    power = np.linspace(-3.0, 2.0, T)
    fm = np.asfortranarray(np.vstack([power[None, :], X.T]))          # (2D+1, T)
    refs = [ft.reference(X[b:b + L]) for b in range(0, T, L)]
    assert [r[0].shape[0] for r in refs] == [13, 13, 7]
    host = vc.vc(_conv(vc, mdl, L)[1], fm)                            # (a fresh converter: vc leaves len(c) at the tail's length)
    dev = vc.vc(_conv(vc, mdl, L)[1], torch.from_numpy(np.ascontiguousarray(fm.T)).cuda().t())
    assert dev.is_cuda
    for path, out in (("vc-host", host), ("vc-device", dev.cpu().numpy())):
        assert out.shape == (D + 1, T) and np.array_equal(out[0], power)
        for k, ref in enumerate(refs):
            _check(out[1:, k * L:k * L + ref[0].shape[0]], ref, path, D)
