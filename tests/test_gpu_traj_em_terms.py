"""GPU: one pass of the full-covariance trajectory EM (csrc/traj_em.hip: traj_em_post_kernel, traj_em_g_kernel,
traj_em_valu_kernel, traj_em_scan_kernel, traj_em_blend_kernel and the table / index handed to the solvers) term by term, through
the test hook vcmi_debug_traj_em_estep, against the longdouble restatement tests/traj_em_restatement.py (estep_terms) inside its
derived element-wise bounds (estep_bounds; the flag band, check_pass) -- on utterances longer than a workgroup and than the scan's
chunk, on models whose pure and mixed frames lie side by side ("half"), and on frames placed on the pure / mixed decision line.
tests/test_traj_em_terms_host.py asserts on the CPU what this file takes for granted about its inputs and its checker.

Tolerances: every one is a bound of estep_bounds (derived there, none measured on the device); end to end the file
test_gpu_traj_em.py's TOL_SYNTH = 1e-9, which test_traj_em_terms_host.py::test_half_inputs_are_well_conditioned justifies for the
new inputs (a 1e-13 perturbation of X moves y^n by < 1e-11)."""
import ctypes as C
import functools

import numpy as np
import pytest

import traj_em_restatement as R
from conftest import julia_model, relerr

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
TOL_SYNTH = 1e-9
OLD = ["native-20", "padded-13", "cfg5-40", "big-48", "valu-52"]
PATHS = ["mfma", "per-frame"]
PADDED = {13: 16}                     # static dimensions of the cases here that the blocked solver runs in a larger one


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    m.set_devices([])
    return m


def inputs(name):
    """-> model, [X], [reference or None]"""
    if name in R.HALF:
        model, Xs, _ = R.half_inputs(name)
        return model, Xs, R.half_reference(name)
    model, Xs = R.case_inputs(name)
    return model, Xs, R.case_reference(name)


def converter(vc, model, T, em_iters=0):
    return vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*model)), T, em_iters=em_iters)


@functools.lru_cache(maxsize=None)
def bounds(name, u, j):
    model, Xs, refs = inputs(name)
    return R.estep_bounds(model, Xs[u], refs[u]["ys"][j])


@functools.lru_cache(maxsize=None)
def line_bounds(name):
    model, X, y, _ = R.line_inputs(name)
    return R.estep_bounds(model, X, y)


def run_hook(t, model, X, y, pad=0):
    """vcmi_debug_traj_em_estep: X (T,2D), y (T,D) -> the dict check_pass reads (the arrays in the library's memory order: gamma
    (T,M), gbar (T,2D), table (count, 2Ds, 2Ds)), or None where pad = 1 is refused (no padded dimension)"""
    from voiceconversion_jl_amd import _lib
    fn = _lib.lib.vcmi_debug_traj_em_estep
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    fn.argtypes, fn.restype = [C.c_void_p, dp, dp, C.c_int64, C.c_int, dp, dp, ip, dp, lp, ip, dp], C.c_int
    X, y = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    T, K = X.shape
    M = len(model[0])
    Kp = 2 * PADDED.get(K // 2, 46) if pad else K                    # (46: the largest padded dimension there is -- room enough)
    gamma, lse, flag = np.full((T, M), np.nan), np.full(T, np.nan), np.full(T, -7, dtype=np.int32)
    gbar, mh, count = np.full((T, K), np.nan), np.full(T, -7, dtype=np.int64), C.c_int32(-1)
    table = np.full((T, Kp, Kp), np.nan)
    st = fn(t._h, _lib.dptr(X), _lib.dptr(y), T, int(pad), _lib.dptr(gamma), _lib.dptr(lse), flag.ctypes.data_as(ip), _lib.dptr(gbar),
            mh.ctypes.data_as(lp), C.byref(count), _lib.dptr(table))
    if pad and st == _lib.VCMI_ERR_ARG:
        return None
    _lib.check(st)
    n = int(count.value)
    assert 0 <= n <= T and np.all(np.isnan(table[n:]))               # nothing written behind the count
    return dict(gamma=gamma, lse=lse, flag=flag, gbar=gbar, mh=mh, count=n, table=table[:n].copy())


def forced(path):
    """context: the per-frame kernel in place of the MFMA kernels (DBG_TRAJ_G_SCALAR)"""
    from voiceconversion_jl_amd import _lib

    class Ctx:
        def __enter__(self):
            if path == "per-frame":
                _lib.debug_force(_lib.DBG_TRAJ_G_SCALAR)

        def __exit__(self, *a):
            _lib.debug_force(0)

    return Ctx()


def same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def judge(tag, b, out):
    ratios, problems = R.check_pass(b, out)
    print(f"{tag}: error / bound", " ".join(f"{k} {v:.3e}" for k, v in ratios.items()), f"mixed {out['count']}", *problems)
    assert not problems, (tag, problems)
    assert R.accepted(ratios, problems), (tag, ratios)


# ------------------------------------------------------------------------------------------------ 1. the terms of one pass
def _dim(name):
    return R.HALF[name][0] if name in R.HALF else R.CASES[name][1]


@pytest.mark.parametrize("name,path", [(n, p) for n in list(R.HALF) + OLD for p in PATHS if p == "mfma" or 2 * _dim(n) <= 96])
def test_terms_of_one_pass(vc, name, path):
    """gamma per (mixture, frame), lse, gbar and the precision each frame's solver entry points to, inside their bounds at the
    restatement's y^0 and y^2; the flags by the band; mh and count consistent with the flags, mixed indices ascending in frame
    order (check_pass); a repeated call gives the same bits; cond_loglik is the sum of the hook's lse within (T + 16) eps sum
    |lse|; with pad = 1 (static dimension 13, solved in 16) the blended operands of the padded blocked solver hold the same
    matrices and keep the padding's unit diagonal and zeros exactly.  per-frame: the same under DBG_TRAJ_G_SCALAR, which takes
    traj_em_valu_kernel (above 2D = 96 that kernel runs either way: one run)."""
    model, Xs, refs = inputs(name)
    D = Xs[0].shape[1] // 2
    t = converter(vc, model, max(len(X) for X in Xs))
    if D not in PADDED:                                              # a handle without a padded dimension refuses pad = 1
        assert run_hook(t, model, Xs[-1], refs[-1]["ys"][0], pad=1) is None
    with forced(path):
        for u, (X, ref) in enumerate(zip(Xs, refs)):
            if ref is None:
                continue
            for j in (0, 2):
                y = ref["ys"][j]
                b = bounds(name, u, j)
                out = run_hook(t, model, X, y)
                judge(f"{name} {path} T={len(X)} y^{j}", b, out)
                if j == 0:
                    assert same_bits(out, run_hook(t, model, X, y))
                want = float(np.sum(out["lse"]))
                L = t.cond_loglik(np.asfortranarray(X.T), np.asfortranarray(np.asarray(y).T))
                assert abs(L - want) <= (len(X) + 16) * EPS * float(np.sum(np.abs(out["lse"]))), (name, len(X), j, L, want)
                if D in PADDED:
                    padded = run_hook(t, model, X, y, pad=1)
                    assert padded is not None
                    Dp = PADDED[D]
                    keep = np.r_[np.arange(D), Dp + np.arange(D)]
                    tab = padded.pop("table")
                    inner = tab[:, keep][:, :, keep]
                    want_pad = np.zeros((2 * Dp, 2 * Dp))
                    want_pad[np.arange(D, Dp), np.arange(D, Dp)] = 1.0
                    rest = tab.copy()
                    rest[np.ix_(np.arange(len(tab)), keep, keep)] = 0.0
                    assert np.array_equal(rest, np.broadcast_to(want_pad, rest.shape)), float(np.max(np.abs(rest - want_pad)))
                    judge(f"{name} {path} T={len(X)} y^{j} padded", b, dict(padded, table=inner))
                    assert same_bits(padded, {k: v for k, v in out.items() if k != "table"})


# ------------------------------------------------------------------------------------------------ 2. the decision line
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(R.LINE))
def test_decision_line(vc, name, path):
    """Every fourth frame sits at log r_t = -30 .. -45 (r_t: the weight beside the best mixture's), on both sides of where
    em_finish_frame's arithmetic draws the line (r of about max(1, |l_best|) 2^-53; |l_best| of the targets is 408 .. 7426 at
    T = 64 and 265 .. 134414 at T = 130): a frame outside the band must be flagged as the restatement decides, one inside may be either, and whichever it is, its gamma, mh
    and the operands the solver reads must be consistent with the flag and inside their bounds (check_pass)."""
    model, X, y, lev = R.line_inputs(name)
    t = converter(vc, model, len(X))
    with forced(path):
        out = run_hook(t, model, X, y)
        judge(f"{name} {path}", line_bounds(name), out)
        tg = np.flatnonzero(~np.isnan(lev))
        print(f"{name} {path} flags by level:", " ".join(f"{lev[s]:g}:{out['flag'][s]}" for s in tg))
        assert same_bits(out, run_hook(t, model, X, y))


# ------------------------------------------------------------------------------------------------ 3. end to end
@pytest.mark.parametrize("name", list(R.HALF))
def test_half_cases_end_to_end(vc, name):
    """em_iters = 1, 2, 4 against the restatement at TOL_SYNTH; the batch call equals the single calls bit for bit."""
    model, Xs, refs = inputs(name)
    t = converter(vc, model, max(len(X) for X in Xs))
    Xj = [np.asfortranarray(X.T) for X in Xs]
    for n in (1, 2, 4):
        t.em_iters = n
        Ys = t.fvconvert_batch(Xj)
        for x, yy, r in zip(Xj, Ys, refs):
            e = relerr(yy, r["ys"][n].T)
            print(f"{name} T={x.shape[1]} n={n}: {e:.2e}")
            assert e < TOL_SYNTH
        if n == 2:
            for x, yy in zip(Xj, Ys):
                assert np.array_equal(vc.fvconvert(t, x), yy)


def test_the_seven_lengths_cut_into_slices(vc):
    """The batch of half-12 (1100 .. 1 frames, 757 mixed) with the table cap lowered to the model's matrices plus 100 blended
    ones: cut down to single utterances, the same bits as the uncut run."""
    from voiceconversion_jl_amd import _lib
    cap = _lib.lib.vcmi_debug_traj_em_cap
    cap.argtypes, cap.restype = [C.c_void_p, C.c_size_t], C.c_int
    times = _lib.lib.vcmi_debug_traj_em_times
    times.argtypes, times.restype = [C.c_void_p, C.c_int, C.POINTER(C.c_double)], C.c_int
    model, Xs, _ = inputs("half-12")
    t = converter(vc, model, max(len(X) for X in Xs), em_iters=2)
    Xj = [np.asfortranarray(X.T) for X in Xs]
    want, hwant = t.fvconvert_batch(Xj), t.em_history()
    _lib.check(cap(t._h, 8 * (len(model[0]) + 100) * 24 ** 2))
    out = (C.c_double * 8)()
    _lib.check(times(t._h, 1, out))
    got, hgot = t.fvconvert_batch(Xj), t.em_history()
    _lib.check(times(t._h, 0, out))
    _lib.check(cap(t._h, 0))
    assert out[7] > 2, out[7]                                        # more slice-iterations than one slice's two
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    assert np.all(np.abs(hgot - hwant) <= 1e-12 * np.abs(hwant))
