"""CPU: trajectory conversion with three windows (static + delta + delta-delta) from a cross-diagonal model, without a device.
  1. tests/traj_penta_restatement.py: its two statements -- through an explicit W and through the pentadiagonal closed form --
     agree within the tolerance on every shape of the GPU tests, and the preconditions of those tests hold on the actual inputs:
     every q > 0 and no frame's arg-max within rounding of a tie.
  2. tests/c/traj_penta_check.cpp: the solver's per-step header (csrc/traj_penta_step.hpp) run on the CPU over chains of
     T = 1 .. 2000 against a long-double solve, and the invariants of csrc/traj_band_plan.hpp -- a stand-alone program under
     ASan + UBSan, built like tests/test_traj_bdiag_host.py builds its check; nothing is loaded into Python.
  3. push_delta(order=2) and constructW(D, T, windows=3) on the host path against the restatement.
  4. The argument errors that are raised before a device is touched."""
import os
import subprocess

import numpy as np
import pytest

import traj_diag_restatement as DR
import traj_penta_restatement as R
from conftest import ROOT, relerr

OUT = os.path.join(ROOT, "oracle", "_build")
CMD = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "traj_penta_check.cpp")]


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("D,M,Ts,swap", [(D, M, tuple(Ts), False) for D, M, Ts in R.SHAPES + [R.VC_CASE]] + [(12, 4, (1, 2, 3, 4, 5, 50), True)])
def test_dense_w_and_closed_form_agree_and_the_preconditions_hold(D, M, Ts, swap):
    model, Xs = R.make_case(D, M, list(Ts), swap)
    bt = R.PentaTrajectory(*model, swap)
    assert bt.D == D and bt.D2 == 3 * D and np.all(bt.q > 0) and np.all(np.isfinite(bt.q))
    for X in Xs:
        assert X.shape == (X.shape[0], 3 * D)
        gap, bound = bt.undecided(X)
        assert int(np.sum(~(gap > bound))) == 0, (gap.min(), bound.max())
        y, cond, rho = bt.banded(X)
        err, tol = relerr(bt.dense(X), y), DR.tolerance(cond) * rho
        print(f"D={D} M={M} T={X.shape[0]} swap={swap}: relerr {err:.3e}  cond {cond:.3f}  rho {rho:.3f}  bound {tol:.3e}  "
              f"distinct mixtures {len(set(bt.mhat(X)))}")
        assert 1.0 <= cond < 1.0e4 and rho >= 1.0
        assert err < tol
    # the chunks of the vc test are utterances of their own
    if (D, M, list(Ts)) == R.VC_CASE:
        fm = np.concatenate([np.zeros((Ts[0], 1)), Xs[0]], axis=1)
        for b in range(0, Ts[0], 30):
            gap, bound = bt.undecided(fm[b:b + 30, 1:])
            assert int(np.sum(~(gap > bound))) == 0
        out, cond, rho = bt.vc(fm, 30)
        assert out.shape == (Ts[0], D + 1) and relerr(out[:30, 1:], bt.dense(fm[:30, 1:])) < DR.tolerance(cond) * rho


def test_tie_case_is_a_tie_and_only_that():
    model, X = R.tie_case()
    bt = R.PentaTrajectory(*model)
    assert np.all(bt.mhat(X) == 1) and np.all(bt.q[:, :2] > 0)
    a, b = bt.banded(X, mhat=np.ones(10, dtype=np.int64))[0], bt.banded(X, mhat=np.full(10, 2))[0]
    assert relerr(a, b) > 1e-3


# ------------------------------------------------------------------------------------------------ 2. the step header and the plan
def test_step_header_and_plan_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "traj_penta_check_asan")
    subprocess.run(CMD + ["-fsanitize=address,undefined", "-o", exe], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout)
    assert p.returncode == 0 and "traj_penta_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    chains = [line.split() for line in p.stdout.splitlines() if line.startswith("chain T ")]
    assert {int(c[2]) for c in chains} == {1, 2, 3, 4, 5, 50, 2000}


# ------------------------------------------------------------------------------------------------ 3. push_delta and constructW
@pytest.mark.parametrize("T", [1, 2, 3, 7])
def test_push_delta_order_2_and_constructw_3_on_the_host(T):
    import voiceconversion_jl_amd as vc
    D = 5
    src = np.random.default_rng(40 + T).standard_normal((T, D))
    want = R.push_delta2(src)
    got = vc.push_delta(np.asfortranarray(src.T), order=2)
    assert got.shape == (3 * D, T) and got.flags.f_contiguous
    assert np.array_equal(got, want.T)
    assert np.array_equal(got[:2 * D], vc.push_delta(np.asfortranarray(src.T)))             # bit for bit the two-window rows
    assert np.array_equal(vc.push_delta(np.asfortranarray(src.T), order=1), vc.push_delta(src.T))
    # the edges, spelt out
    a = got[2 * D:]
    assert np.array_equal(a[:, 0], -2.0 * src[0] + (src[1] if T > 1 else 0.0))
    if T > 1:
        assert np.array_equal(a[:, -1], src[-2] + -2.0 * src[-1])
    # W: the package's against the restatement's, and W x = the delta-delta rows (and the delta rows inside the utterance)
    W = vc.constructW(D, T, windows=3)
    assert W.shape == (3 * D * T, D * T) and np.array_equal(W.toarray(), R.construct_w(D, T))
    wx = (W @ src.reshape(-1)).reshape(T, 3 * D)
    assert np.array_equal(wx[:, :D], src)
    assert np.allclose(wx[:, 2 * D:], want[:, 2 * D:], rtol=0, atol=4 * 2.0 ** -52 * np.abs(src).max())
    assert np.allclose(wx[1:-1, D:2 * D], want[1:-1, D:2 * D], rtol=0, atol=2.0 ** -52 * np.abs(src).max())
    # two windows: unchanged, also when named
    W2 = vc.constructW(D, T)
    assert W2.shape == (2 * D * T, D * T) and np.array_equal(W2.toarray(), vc.constructW(D, T, windows=2).toarray())
    assert np.array_equal(W.toarray().reshape(T, 3, D, T * D)[:, :2].reshape(2 * D * T, D * T), W2.toarray())


# ------------------------------------------------------------------------------------------------ 4. argument errors
def test_argument_errors_before_a_device_is_touched():
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import _lib
    assert {"vcmi_traj_create_bdiag_windows", "vcmi_traj_get_windows", "vcmi_push_delta2", "vcmi_push_delta2_dev"} <= set(_lib.SIGNATURES)
    x = np.zeros((3, 4), order="F")
    for order in (0, 3, -1, None, "2"):
        with pytest.raises(ValueError, match="order"):
            vc.push_delta(x, order=order)
    for windows in (1, 4, 0):
        with pytest.raises(ValueError, match="windows"):
            vc.constructW(3, 4, windows=windows)
    for g in (None, object(), "model", 3):
        with pytest.raises(TypeError, match="BlockDiagGMMMap"):
            vc.BlockDiagTrajectoryGMMMap(g, 10, windows=3)
    assert _lib.lib.vcmi_traj_get_windows(None) == -1
    import ctypes as C
    h = C.c_void_p()
    assert _lib.lib.vcmi_traj_create_bdiag_windows(None, 10, 3, C.byref(h)) != 0 and not h
    assert _lib.lib.vcmi_push_delta2(None, 3, 4, _lib.dptr(x)) != 0
    assert _lib.lib.vcmi_push_delta2_dev(None, 3, 0, 4, None, 9, None) != 0                 # D < 1: refused before any device call
