"""GPU: BlockDiagTrajectoryEMGMMMap -- EM re-estimation over all mixtures for a trajectory converter made straight from a
cross-diagonal model (vcmi_traj_set_em_bdiag, vcmi_traj_cond_loglik_bdiag[_dev]: the fused E-step + M-step sums of
csrc/traj_em_bdiag.hip and the tridiagonal solver of csrc/traj_diag.hip over the per-frame table) -- against the numpy restatement
tests/traj_em_bdiag_restatement.py and against the detour through the expanded model.

Every tolerance is one of the restatement's bounds (derived in its docstring): (1)-(3) element-wise for lse, qbar and gbar of one
fused pass, (5) for y^k, (6) for the objective.  tests/test_traj_em_bdiag_host.py asserts for every input used here that every
q > 0, that every frame is mixed, that the first iteration moves y by at least 1 % of max |y| (a converter that ignored em_iters
fails the parity tests) and that the E/M map contracts."""
import ctypes as C
import functools

import numpy as np
import pytest

import traj_em_bdiag_restatement as E
from conftest import relerr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def _conv(vc, model, T, em_iters):
    return vc.BlockDiagTrajectoryEMGMMMap(vc.BlockDiagGMMMap(*model), T, em_iters=em_iters)


def _detour(vc, model, T, em_iters):
    w, mu, cov = model
    return vc.TrajectoryGMMMap(vc.GMMMap(w, mu, vc.expand_block_diag(cov)), T, em_iters=em_iters)


def _with_an_empty_one(Xs):
    """the batch with an empty utterance in second place -> (batch of (2D,T) matrices, positions of the real ones)"""
    D2 = Xs[0].shape[1]
    batch = [X.T for X in Xs[:1]] + [np.zeros((D2, 0), order="F")] + [X.T for X in Xs[1:]]
    return batch, [0] + list(range(2, len(Xs) + 1))


@functools.lru_cache(maxsize=None)
def _term_bounds(name, u, j):
    (w, mu, cov), Xs = E.case_inputs(name)
    return E.estep_bounds((w, mu, cov, False), Xs[u], E.case_reference(name)[u]["ys"][j])


def _estep_hook(t, X, y):
    """one fused pass at y: X (T,2D), y (T,D) -> lse (T), qbar (T,2D), gbar (T,2D)"""
    from voiceconversion_jl_amd import _lib
    fn = _lib.lib.vcmi_debug_traj_em_bdiag_estep
    dp = C.POINTER(C.c_double)
    fn.argtypes, fn.restype = [C.c_void_p, dp, dp, C.c_int64, dp, dp, dp], C.c_int
    X, y = np.ascontiguousarray(X), np.ascontiguousarray(y)
    T = X.shape[0]
    lse, qbar, gbar = np.empty(T), np.empty_like(X), np.empty_like(X)
    _lib.check(fn(t._h, _lib.dptr(X), _lib.dptr(y), T, _lib.dptr(lse), _lib.dptr(qbar), _lib.dptr(gbar)))
    return lse, qbar, gbar


# ------------------------------------------------------------------------------------------------ 1. the terms of one pass
@pytest.mark.parametrize("name", list(E.CASES))
def test_terms_of_one_fused_pass(vc, name):
    """lse_t, qbar and gbar of one pass at the restatement's y^0 and y^2, element-wise inside bounds (2) and (3) around the
    longdouble evaluation; cond_loglik on host matrices and on device tensors against sum_t lse_t within sum_t BL_t plus the
    (T + 16) eps sum |lse_t| of the summation.  The shapes: 2D = 80 over five tiles; one to five frames; padded tables (2D = 14);
    63, 64, 65, 129 frames (the stencil across a tile edge); a mixture without weight; the largest dimension; 256 mixtures; and the
    kernel's 32-frame tiles (small-tile-*)."""
    import torch
    model, Xs = E.case_inputs(name)
    t = _conv(vc, model, max(len(X) for X in Xs), 0)
    for u, (X, ref) in enumerate(zip(Xs, E.case_reference(name))):
        for j in (0, 2):
            y = ref["ys"][j]
            b = _term_bounds(name, u, j)
            lse, qbar, gbar = _estep_hook(t, X, y)
            for key, got in (("lse", lse), ("qbar", qbar), ("gbar", gbar)):
                err = np.abs(got - np.asarray(b["ref"][key], dtype=np.float64))
                print(f"{name} T={len(X)} y^{j} {key}: largest error / bound {float(np.max(err / b[key])):.3e}")
                assert np.all(err <= b[key]), (name, len(X), j, key, float(np.max(err / b[key])))
            want = float(b["ref"]["L"])
            Lb = float(b["lse"].sum()) + (len(X) + 16) * EPS * float(np.abs(b["ref"]["lse"]).sum())
            Lh = t.cond_loglik(np.asfortranarray(X.T), np.asfortranarray(y.T))
            dX, dY = (torch.from_numpy(np.ascontiguousarray(a)).cuda().t() for a in (X, y))
            Ld = t.cond_loglik(dX, dY)
            assert Ld.is_cuda and float(Ld.cpu()[0]) == Lh
            assert abs(Lh - want) <= Lb, (name, len(X), j, Lh, want, Lb)
    assert t.em_iters == 0 and t.cond_loglik(np.zeros((2 * E.CASES[name][0], 0), order="F"), np.zeros((E.CASES[name][0], 0), order="F")) == 0.0


# ------------------------------------------------------------------------------------------------ 2. one step
@pytest.mark.parametrize("name", list(E.CASES))
def test_one_pair(vc, name):
    """em_iters = 1 against one restated pair within bound (5) at k = 1, which is the one-step bound (4) plus what the pair makes
    of the arg-max solve's 64 cond rho eps.  y^1 is 1.2 .. 40 % of max |y| away from y^0: a kernel that ignored the setting fails."""
    model, Xs = E.case_inputs(name)
    t = _conv(vc, model, max(len(X) for X in Xs), 1)
    assert t.em_iters == 1 and t.precision == "diag"
    Ys = t.fvconvert_batch([X.T for X in Xs])
    assert len(t.em_history()) == 1
    for X, y, ref in zip(Xs, Ys, E.case_reference(name)):
        err = relerr(y, ref["ys"][1].T)
        print(f"{name} T={len(X)}: relerr {err:.3e}  bound {ref['bound'][1]:.3e}  (to y^0: {relerr(y, ref['ys'][0].T):.3e})")
        assert err < ref["bound"][1], (name, len(X), err, ref["bound"][1])


# ------------------------------------------------------------------------------------------------ 3. end to end
@pytest.mark.parametrize("name", list(E.CASES))
def test_four_pairs_end_to_end(vc, name):
    """em_iters = 4: y^4 within bound (5), em_history() (summed over the utterances) within the sum of bounds (6); an empty
    utterance rides in the batch; batch equals single, bit for bit, and the single call's history is its utterance's"""
    model, Xs = E.case_inputs(name)
    refs = E.case_reference(name)
    t = _conv(vc, model, max(len(X) for X in Xs), E.NITER)
    batch, real = _with_an_empty_one(Xs)
    Ys = t.fvconvert_batch(batch)
    hist = t.em_history()
    assert Ys[1].shape == (E.CASES[name][0], 0) and len(hist) == E.NITER
    for X, k, ref in zip(Xs, real, refs):
        err = relerr(Ys[k], ref["ys"][E.NITER].T)
        print(f"{name} T={len(X)}: relerr {err:.3e}  bound {ref['bound'][E.NITER]:.3e}")
        assert err < ref["bound"][E.NITER], (name, len(X), err, ref["bound"][E.NITER])
    for j in range(E.NITER):
        want, bound = sum(r["L"][j] for r in refs), sum(r["Lbound"][j] for r in refs)
        print(f"{name} L_{j}: {hist[j]:.12g} against {want:.12g}, bound {bound:.2e}")
        assert abs(hist[j] - want) <= bound, (name, j, hist[j], want, bound)
    for X, k, ref in zip(Xs, real, refs):
        assert np.array_equal(vc.fvconvert(t, X.T), Ys[k])
        h1 = t.em_history()
        assert len(h1) == E.NITER and all(abs(h1[j] - ref["L"][j]) <= ref["Lbound"][j] for j in range(E.NITER))


# ------------------------------------------------------------------------------------------------ 4. against the detour
@pytest.mark.parametrize("name,k", [("tiles-12-4", 2), ("40-8", 2), ("tiles-12-4", 4)])
def test_against_the_detour_through_the_expanded_model(vc, name, k):
    """TrajectoryGMMMap(GMMMap(w, mu, expand_block_diag(covars)), T, em_iters=k), both sides on the device, within twice bound (5)
    (each is within one of the exact trajectory)"""
    model, Xs = E.case_inputs(name)
    batch = [X.T for X in Xs]
    T = max(len(X) for X in Xs)
    new = _conv(vc, model, T, k).fvconvert_batch(batch)
    old = _detour(vc, model, T, k).fvconvert_batch(batch)
    for X, a, b, ref in zip(Xs, new, old, E.case_reference(name)):
        err = relerr(a, b)
        print(f"{name} T={len(X)} k={k}: relerr {err:.3e}  bound {2 * ref['bound'][k]:.3e}")
        assert err < 2 * ref["bound"][k], (name, len(X), k, err)


# ------------------------------------------------------------------------------------------------ 5. em_iters = 0
def test_without_iterations_it_is_the_plain_converter(vc):
    model, Xs = E.case_inputs("tiles-12-4")
    batch, _ = _with_an_empty_one(Xs)
    plain = vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(*model), 129).fvconvert_batch(batch)
    t = _conv(vc, model, 129, 0)
    got = t.fvconvert_batch(batch)
    assert t.em_iters == 0 and len(t.em_history()) == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, plain))
    t.em_iters = 3
    moved = t.fvconvert_batch(batch)
    assert len(t.em_history()) == 3 and relerr(moved[0], plain[0]) > 1e-2
    t.em_iters = 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(t.fvconvert_batch(batch), plain)) and len(t.em_history()) == 0


# ------------------------------------------------------------------------------------------------ 6. bits
def test_bits_do_not_depend_on_the_batch_the_stream_or_earlier_calls(vc):
    """tiles-12-4 with two iterations: the batch composition (another order, a subset, single calls), a repeat, a second stream,
    other converters in between (the detour, a cross-diagonal EM converter of another shape, the same model's frame-by-frame
    entry), and the order em_iters was toggled in"""
    import torch
    model, Xs = E.case_inputs("tiles-12-4")
    batch = [X.T for X in Xs]
    t = _conv(vc, model, 129, 2)
    first, hist = t.fvconvert_batch(batch), t.em_history()
    again = t.fvconvert_batch(batch)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, first)) and np.array_equal(t.em_history(), hist)
    order = [3, 0, 4, 2, 1]
    shuffled = t.fvconvert_batch([batch[i] for i in order])
    assert all(shuffled[k].tobytes() == first[i].tobytes() for k, i in enumerate(order))
    # (the history sums the five utterances in the caller's order: another order moves it by at most 8 eps of the absolute sum)
    Labs = np.array([sum(abs(r["L"][j]) for r in E.case_reference("tiles-12-4")) for j in range(2)])
    assert np.all(np.abs(t.em_history() - hist) <= 8 * EPS * 1.001 * Labs)
    subset = t.fvconvert_batch(batch[1:3])
    assert subset[0].tobytes() == first[1].tobytes() and subset[1].tobytes() == first[2].tobytes()
    assert all(vc.fvconvert(t, x).tobytes() == y.tobytes() for x, y in zip(batch, first))
    other_model, other_Xs = E.case_inputs("7-2")
    others = [lambda: _detour(vc, model, 129, 1).fvconvert_batch(batch[:2]),
              lambda: _conv(vc, other_model, 30, 3).fvconvert_batch([X.T for X in other_Xs]),
              lambda: vc.fvconvert(t.gmmmap, np.asfortranarray(Xs[0].T))]
    for other in others:
        other()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(t.fvconvert_batch(batch), first))
    # a second stream, through the device entry of vc
    fm = np.asfortranarray(np.vstack([np.arange(129.0)[None, :], Xs[3].T]))
    dfm = torch.from_numpy(np.ascontiguousarray(fm.T)).cuda().t()
    t129 = _conv(vc, model, 129, 2)
    dev0 = vc.vc(t129, dfm).cpu().numpy()
    assert np.array_equal(dev0[1:], first[3])
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        dev1 = vc.vc(t129, dfm)
    s1.synchronize()
    assert np.array_equal(dev1.cpu().numpy(), dev0)
    # toggles: 2 -> 0 -> 4 -> 2 and a handle that was made with 4 and set to 2
    t.em_iters = 0
    t.fvconvert_batch(batch)
    t.em_iters = 4
    four = t.fvconvert_batch(batch)
    t.em_iters = 2
    assert all(a.tobytes() == b.tobytes() for a, b in zip(t.fvconvert_batch(batch), first))
    t2 = _conv(vc, model, 129, 4)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(t2.fvconvert_batch(batch), four))
    t2.em_iters = 2
    assert all(a.tobytes() == b.tobytes() for a, b in zip(t2.fvconvert_batch(batch), first))


# ------------------------------------------------------------------------------------------------ 7. the vc surface
def test_vc_and_vc_batch_convert_chunk_by_chunk(vc):
    """vc-12-4, T = 100 in chunks of len(c) = 30 with two iterations: host matrices and device tensors, with and without
    delta=True, every chunk equal to fvconvert of that chunk bit for bit (y^2 within bound (5) of the restatement of the chunk
    follows from test 3's property: an utterance's bits do not depend on the call); the post-filter over the whole converted
    utterance equal to the library's own filter of the unfiltered result, on every path the same bits"""
    import torch
    from oracle import np_oracle as npo
    D, M, (T,), _ = E.CASES["vc-12-4"]
    L, k = 30, 2
    model, (X,) = E.case_inputs("vc-12-4")
    power = np.linspace(-3.0, 2.0, T)
    static = np.concatenate([power[:, None], X[:, :D]], axis=1)               # (T, D+1)
    full = np.concatenate([power[:, None], X], axis=1)                         # (T, 2D+1)
    assert np.array_equal(npo.push_delta(static[:, 1:]), X)
    fresh = lambda: _conv(vc, model, L, k)                                     # noqa: E731  (vc leaves len(c) at the tail's length)
    chunks = [vc.fvconvert(fresh(), np.asfortranarray(X[b:b + L].T)) for b in range(0, T, L)]
    want = np.concatenate(chunks, axis=1)
    ref0 = E.em_convert((*model, False), X[:L], k)
    assert relerr(chunks[0], ref0["ys"][k].T) < ref0["bound"][k] and relerr(chunks[0], ref0["ys"][0].T) > 1e-2
    c = fresh()
    out = vc.vc(c, np.asfortranarray(full.T))
    assert np.array_equal(out[0], full[:, 0]) and len(c) == 10 and c.em_iters == k
    assert np.array_equal(out[1:], want)
    assert np.array_equal(vc.vc(fresh(), np.asfortranarray(static.T), delta=True), out)
    dstatic = torch.from_numpy(static.copy()).cuda().t()
    dfull = torch.from_numpy(full.copy()).cuda().t()
    outd = vc.vc(fresh(), dstatic, delta=True)
    assert outd.is_cuda and np.array_equal(outd.cpu().numpy(), out) and np.array_equal(vc.vc(fresh(), dfull).cpu().numpy(), out)
    # the post-filter
    vs = vc.VarianceScaling(np.var(want, axis=1, ddof=1) * np.linspace(0.5, 2.0, D))
    filtered = vc.fvpostf(vs, outd[1:]).cpu().numpy()
    outf = vc.vc(fresh(), np.asfortranarray(static.T), postfilter=vs, delta=True)
    assert np.array_equal(outf[0], full[:, 0]) and np.array_equal(outf[1:], filtered)
    assert np.array_equal(vc.vc(fresh(), np.asfortranarray(full.T), postfilter=vs), outf)
    assert np.array_equal(vc.vc(fresh(), dstatic, postfilter=vs, delta=True).cpu().numpy(), outf)
    # vc_batch of three utterances, one of them empty: the single call bit for bit, on host matrices and device tensors
    fms = [np.asfortranarray(static.T), np.zeros((D + 1, 0), order="F"), np.asfortranarray(static[:37].T)]
    for pf in (None, vs):
        c = fresh()
        outs = vc.vc_batch(c, fms, postfilter=pf, delta=True)
        assert len(c) == L and outs[1].shape == (D + 1, 0)
        for u in (0, 2):
            assert np.array_equal(outs[u], vc.vc(fresh(), fms[u], postfilter=pf, delta=True)), (pf is not None, u)
        douts = vc.vc_batch(fresh(), [torch.from_numpy(np.ascontiguousarray(f.T)).cuda().t() for f in fms], postfilter=pf, delta=True)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(douts, outs))
    assert np.array_equal(vc.vc_batch(fresh(), fms, delta=True)[0], out)


# ------------------------------------------------------------------------------------------------ 8. what is refused
def test_refusals_leave_a_working_handle(vc):
    from voiceconversion_jl_amd import _lib
    model, Xs = E.case_inputs("12-4")
    refs = E.case_reference("12-4")
    X = np.asfortranarray(Xs[-1].T)
    t = _conv(vc, model, 50, 1)

    def still_converts(tt=t, k=1):
        assert tt.em_iters == k and relerr(vc.fvconvert(tt, X), refs[-1]["ys"][k].T) < refs[-1]["bound"][k]

    # the new entry on a dense handle; a negative count
    w, mu, cov = model
    dense = vc.TrajectoryGMMMap(vc.GMMMap(w, mu, vc.expand_block_diag(cov)), 50)
    want_dense = vc.fvconvert(dense, X)
    with pytest.raises(vc.VCMIError, match="cross-diagonal"):
        _lib.check(_lib.lib.vcmi_traj_set_em_bdiag(dense._h, 1))
    L = C.c_double(0.0)
    Y = np.asfortranarray(refs[-1]["ys"][0].T)
    with pytest.raises(vc.VCMIError, match="cross-diagonal"):
        _lib.check(_lib.lib.vcmi_traj_cond_loglik_bdiag(dense._h, _lib.dptr(X), _lib.dptr(Y), 50, C.byref(L)))
    assert dense.em_iters == 0 and np.array_equal(vc.fvconvert(dense, X), want_dense)
    with pytest.raises(vc.VCMIError, match="negative"):
        t.em_iters = -1
    still_converts()
    # a GV converter over it: refused at all four convert entries while em_iters > 0 (the message names EM), converts at 0
    muv = np.var(refs[-1]["ys"][0], axis=0, ddof=1) * 1.2
    tgv = vc.DiagTrajectoryGVGMMMap(t, muv, np.diag(muv ** 2 * 0.1))
    fm = np.asfortranarray(np.vstack([np.ones((1, 50)), X]))
    for call in (lambda: vc.fvconvert(tgv, X, epochs=3), lambda: vc.vc(tgv, fm), lambda: tgv._vc(fm, vc.VarianceScaling(muv)),
                 lambda: vc.vc_batch(tgv, [fm, fm])):
        with pytest.raises(vc.VCMIError, match="EM"):
            call()
    still_converts()
    t.em_iters = 0
    plain = vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(*model), 50)
    gv_plain = vc.DiagTrajectoryGVGMMMap(plain, muv, np.diag(muv ** 2 * 0.1))
    assert np.array_equal(vc.fvconvert(tgv, X, epochs=3), vc.fvconvert(gv_plain, X, epochs=3))
    t.em_iters = 1
    still_converts()
    # the plain converter keeps refusing both
    with pytest.raises(vc.VCMIError, match="diagonal"):
        plain.em_iters = 1
    with pytest.raises(vc.VCMIError, match="cross-diagonal"):
        plain.cond_loglik(X, Y)
    assert plain.em_iters == 0 and np.array_equal(vc.fvconvert(plain, X), vc.fvconvert(_conv(vc, model, 50, 0), X))
    # only a BlockDiagGMMMap makes one
    with pytest.raises(TypeError, match="BlockDiagGMMMap"):
        vc.BlockDiagTrajectoryEMGMMMap(dense.gmmmap, 50)
