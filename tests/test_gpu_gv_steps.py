"""GPU: ONE EPOCH of the GV ascent (csrc/traj_gv.hip: traj_gv2_kernel, traj_gv_kernel, traj_gvw_kernel) at a time, each
gradient summand visible -- the step check.

The other GV tests compare the final trajectory with the oracle at 1e-6 of max |y| and the reference's alpha = 1e-5, where the
whole ascent is 1e-5 .. 1e-3 of y and its GV term 1e-9: they cannot see what an epoch computes.  Here, for epoch counts n,

    y_n = fvconvert(tgv, X, epochs=n, alpha),  y_{n+1} = the same call with n + 1      (the ascent is deterministic: the n call is
                                                                                        repeated and must give the same bits)
    | (y_{n+1} - y_n) - alpha (lik + gv)(y_n) |  <=  bar        element by element,

with the right-hand gradient from tests/gv_restatement.py in long double AT THE DEVICE'S OWN y_n: whatever the trajectory solve
and the earlier epochs did cancels, and one epoch of kernel arithmetic is what is measured.  The inputs (gv_restatement.py's
cases) make both summands at least a fifth of every checked step and the step at least 1e-5 of y, and every mutant of the epoch
listed there misses the bar at least a hundredfold (tests/test_gv_restatement_host.py, from the oracle alone).

The bar -- derived, not measured on the kernel:

    bar = K 2^-53 ( |y_n| + |y_{n+1}| + alpha (lik_mag + gv_mag) ),     K = 3 * 2D + T + D + 16.

An FP64 sum of k terms is off by at most gamma_k = k 2^-53 / (1 - k 2^-53) times the sum of the terms' absolute values, in any
order of summation (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 and 4.2); a product adds one 2^-53, a fused
multiply-add none.  lik_mag and gv_mag are the summands with every product and addend replaced by its absolute value, so a right
kernel's gradient is within (longest chain) 2^-53 (lik_mag + gv_mag) of the exact one.  The chain of one element of dy: u = W y
(2 terms), v = Q u (2D), the stencil W' v (3) -- bounded by 3 * 2D together, and the same for r = W' D^-1 E, which is added, not
chained; the moments mean and var_1, sums over T frames; the product Sigma_vv^-1' (var_1 - mu_v), D terms.  The errors of the
moments enter the gradient through products whose magnitudes gv_mag already holds, so the lengths add: 3 * 2D + T + D.  The
stated constant 16 covers what that count leaves out: the shifted two-level reduction of the moments (S1, S2 about the previous
mean: (S2 - S1^2 / T) / (T - 1), mean += S1 / T), omega, -2/T, y - mean, the two additions that form dy and the update
fma(alpha, dy, y_n).  |y_n| + |y_{n+1}| carries the rounding of the stored y_{n+1} (2^-53 |y_{n+1}|) and lets the difference of
two stored doubles be taken against numbers of their own size.  The restatement's own error, K 2^-63-ish, is 2^-10 of this.
Not in the count: the device prepares Q_m, A_m and Sigma_vv^-1 with its own FP64 inverses, the restatement takes numpy's; the
models are conditioned <= 10 so that this difference, cond 2^-53 of |Q|, stays a small part of K 2^-53 |Q| |u|.

At n = 0 eq. (58) has just made var_1(y) = mu_v: the GV term is zero to rounding, |alpha gv| <= its own share of the bar, which
is asserted as such -- one step from the start says nothing about that term."""
import functools

import numpy as np
import pytest

import gv_restatement as gr
from conftest import julia_model
from gv_restatement import EPS, LD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def _converter(vc, case, L):
    inp = gr.inputs(case)
    t = vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*inp["model"])), L)
    return vc.TrajectoryGVGMMMap(t, inp["muv"], np.asfortranarray(inp["Sv"]))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_steps(case, convert, label):
    """convert(n) -> y_n (D,T) of the case's utterance; the step check at every n of case.ns.  Returns the worst error / bar."""
    p = gr.inputs(case)["pieces"]
    D, T, alpha = case.D, case.T, case.alpha
    ys = {n: convert(n) for n in sorted(set(case.ns) | {n + 1 for n in case.ns})}
    K = gr.chain_length(D, T)
    worst = 0.0
    for n in case.ns:
        assert _same_bits(convert(n), ys[n]), f"{label}: epochs={n} twice gives different bits"
        y_n, y_n1 = np.asarray(ys[n]).T, np.asarray(ys[n + 1]).T
        assert y_n.shape == (T, D) and np.all(np.isfinite(y_n)) and np.all(np.isfinite(y_n1))
        lik, gv, lik_mag, gv_mag = gr.gradient_terms(p, y_n)
        bar = gr.step_bar(D, T, alpha, y_n, y_n1, lik_mag, gv_mag)
        err = np.abs((y_n1.astype(LD) - y_n.astype(LD)) - LD(alpha) * (lik + gv))
        ratio = float(np.max(err / bar))
        step = float(np.max(np.abs(y_n1 - y_n)) / np.max(np.abs(y_n)))
        print(f"GVSTEP {label} {case.id} alpha={alpha:g} n={n}: error/bar {ratio:.2e}  (step {step:.2e} of max|y|, K = {K})")
        if n == 0:      # the GV term is zero by construction at the start
            assert np.all(alpha * np.abs(gv) <= K * EPS * alpha * gv_mag), f"{label}: the GV term at the eq. (58) start"
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{label} {case.id} n={n}: error / bar = {ratio:.3g}"
    return worst


def _single(vc, case, tgv):
    XT = np.asfortranarray(gr.inputs(case)["X"].T)
    return lambda n: vc.fvconvert(tgv, XT, epochs=n, alpha=case.alpha)


@pytest.mark.parametrize("case", gr.GV2_CASES, ids=lambda c: c.id)
def test_two_team_kernel(vc, case):
    """traj_gv2_kernel, the default for 2D <= 96"""
    assert 2 * case.D <= 96 and gr.gv2_lds_bytes(case.D, case.M, case.T) <= gr.LDS_LIMIT
    _check_steps(case, _single(vc, case, _converter(vc, case, case.T)), "gv2")


@pytest.mark.parametrize("case", gr.ONE_TEAM_CASES, ids=lambda c: c.id)
def test_one_team_kernel_forced(vc, case):
    """traj_gv_kernel through the debug hook"""
    from voiceconversion_jl_amd import _lib
    tgv = _converter(vc, case, case.T)
    _lib.debug_force(_lib.DBG_GV_ONE_TEAM)
    try:
        _check_steps(case, _single(vc, case, tgv), "gv1-forced")
    finally:
        _lib.debug_force(0)


def test_one_team_kernel_long_utterance(vc):
    """traj_gv_kernel without the hook: the frame permutation of 29313 frames at D = 12, M = 4 no longer fits the LDS of
    traj_gv2_kernel (the launch rule of traj_gv_launch, restated in gv_restatement.gv2_lds_bytes)"""
    case = gr.LONG_CASE
    assert gr.gv2_lds_bytes(case.D, case.M, case.T) > gr.LDS_LIMIT and max(case.ns) + 1 <= 3 and case.D == 12
    _check_steps(case, _single(vc, case, _converter(vc, case, case.T)), "gv1-long")


@pytest.mark.parametrize("case", gr.GVW_CASES, ids=lambda c: c.id)
def test_wide_kernel(vc, case):
    """traj_gvw_kernel, 2D > 96; T = 1100: the frame permutation beyond the kernel's 1024 LDS slots"""
    assert 2 * case.D > 96
    if case.T == 1100:
        assert ((case.T + 15) // 16 + case.M) * 16 > 1024 and max(case.ns) + 1 <= 3
    _check_steps(case, _single(vc, case, _converter(vc, case, case.T)), "gvw")


def test_batch_members(vc):
    """three utterances of different lengths in ONE fvconvert_batch call (a workgroup loop shared by the members): the step
    check on every member"""
    cases = gr.BATCH_CASES
    assert len({c.T for c in cases}) == 3 and len({(c.D, c.M, c.alpha, c.cov_scale) for c in cases}) == 1
    tgv = _converter(vc, cases[0], max(c.T for c in cases))
    XTs = [np.asfortranarray(gr.inputs(c)["X"].T) for c in cases]

    def batch(n):
        return tgv.fvconvert_batch(XTs, epochs=n, alpha=cases[0].alpha)

    first = functools.lru_cache(maxsize=None)(batch)
    for i, c in enumerate(cases):
        seen = set()

        def convert(n, i=i, seen=seen):        # the first request for n: the shared call; the repeat: a call of its own
            if n in seen:
                return batch(n)[i]
            seen.add(n)
            return first(n)[i]

        _check_steps(c, convert, f"batch[{i}]")
