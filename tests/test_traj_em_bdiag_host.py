"""CPU: the restatement tests/traj_em_bdiag_restatement.py before the device is judged by it (tests/test_gpu_traj_em_bdiag.py), and
the launch rule csrc/traj_em_bdiag_plan.hpp.

  * against the DENSE restatement (tests/traj_em_restatement.em_convert on the expanded model) for the cases with D <= 40, M <= 8,
    over four iterations, within the helper's own k-step bound (5) and objective bound (6).  Measured here: y within 1.1e-14 of
    the dense restatement (relerr), L within 1.9e-14 relative; the largest error / bound ratio is printed per utterance: for y 2.3e-2
    at the arg-max solution y^0 and 7.4e-5 from y^1 on, for L 4.3e-3 and 1.5e-5;
  * the conditions the GPU tests rest on, for every utterance of every case: every q > 0; L non-decreasing over four iterations
    (1e-12 |L| allowed); at least 90 % of the frames mixed at the first E-step (1 - max gamma >= 2^-53; it is 100 %); y moves by at
    least 1 % of max |y| in the first iteration (1.2 .. 40 %), so a converter that ignored em_iters fails the parity tests; the
    doubled amplification kappa <= 2;
  * a float64 evaluation in a second operation order (descending k, descending m) stays inside the per-term bounds (1)-(3);
  * tests/c/traj_em_bdiag_plan_check.cpp under ASan + UBSan, and its rule lines against the rule restated here."""
import os
import subprocess

import numpy as np
import pytest

import traj_bdiag_restatement as R
import traj_em_bdiag_restatement as E
import traj_em_restatement as ER
from conftest import ROOT, relerr

OUT = os.path.join(ROOT, "oracle", "_build")


@pytest.mark.parametrize("name", E.DENSE_CASES)
def test_agrees_with_the_dense_restatement_on_the_expanded_model(name):
    (w, mu, cov), Xs = E.case_inputs(name)
    dense_model = R.expanded_model(w, mu, cov)
    for X, ref in zip(Xs, E.case_reference(name)):
        d = ER.em_convert(*dense_model, X, E.NITER)
        for j in range(E.NITER + 1):
            err, bound = relerr(ref["ys"][j], d["ys"][j]), ref["bound"][j]
            lerr, lbound = abs(ref["L"][j] - d["L"][j]), ref["Lbound"][j]
            print(f"{name} T={len(X)} y^{j}: relerr {err:.2e} bound {bound:.2e} ratio {err / bound:.1e};  L: {lerr:.2e} bound {lbound:.2e} "
                  f"ratio {lerr / lbound:.1e}")
            assert err < bound, (name, len(X), j, err, bound)
            assert lerr < lbound, (name, len(X), j, lerr, lbound)


@pytest.mark.parametrize("name", list(E.CASES))
def test_conditions_the_gpu_tests_rest_on(name):
    (w, mu, cov), Xs = E.case_inputs(name)
    assert np.all(E.Model(w, mu, cov).q > 0)
    for X, ref in zip(Xs, E.case_reference(name)):
        L = np.array(ref["L"])
        assert np.all(np.diff(L) >= -1e-12 * np.abs(L[:-1])), (name, len(X), L)
        mixed = float(np.mean(1.0 - ref["gamma0"].max(axis=1) >= 2.0 ** -53))
        move = relerr(ref["ys"][1], ref["ys"][0])
        kap = max(k[0] for k in ref["kappa"])
        print(f"{name} T={len(X)}: mixed {mixed:.2f}  first move {move:.3e}  kappa undoubled {max(k[1] for k in ref['kappa']):.3f}  "
              f"bound y^4 {ref['bound'][-1]:.2e} = {ref['bound'][-1] / max(ref['step']):.1f} largest single steps")
        assert mixed >= 0.9, (name, len(X), mixed)
        assert move >= 0.01, (name, len(X), move)
        assert kap <= 2.0, (name, len(X), kap)


@pytest.mark.parametrize("name", list(E.CASES))
def test_a_second_operation_order_stays_inside_the_term_bounds(name):
    """at y^0 and y^2: float64, sums over k and m descending, against the longdouble evaluation"""
    (w, mu, cov), Xs = E.case_inputs(name)
    md = E.Model(w, mu, cov)
    for X, ref in zip(Xs, E.case_reference(name)):
        for j in (0, 2):
            b = E.estep_bounds((w, mu, cov, False), X, ref["ys"][j])
            got = md.estep(X, ref["ys"][j], reverse=True)
            live = np.isfinite(b["ell"])
            with np.errstate(invalid="ignore"):                      # (-inf on both sides where w_m <= 0)
                ell_err = np.abs(got["ell"] - np.asarray(b["ref"]["ell"], dtype=np.float64))
            assert np.all(ell_err[live] <= b["ell"][live]), (name, len(X), j, "ell", float(np.max(ell_err[live] / b["ell"][live])))
            assert np.all(np.isneginf(got["ell"][~live]))
            for key in ("lse", "qbar", "gbar"):
                err = np.abs(got[key] - np.asarray(b["ref"][key], dtype=np.float64))
                assert np.all(err <= b[key]), (name, len(X), j, key, float(np.max(err / b[key])))


def _fb(DP, M):
    return 64 if (2 * DP * 65 + M * 64 + 512) * 8 <= 160 * 1024 else 32


def test_launch_rule_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "traj_em_bdiag_plan_check_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "traj_em_bdiag_plan_check.cpp"),
           "-fsanitize=address,undefined", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and "traj_em_bdiag_plan_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    rows = [tuple(int(v) for v in line.split()[1:]) for line in p.stdout.splitlines() if line.startswith("rule ")]
    assert len(rows) == 12 and {r[2] for r in rows} == {32, 64}
    for DP, M, FB, lds in rows:
        assert FB == _fb(DP, M) and lds == (2 * DP * (FB + 1) + M * FB + 512) * 8 <= 160 * 1024
    # the cases of the GPU tests take both tile sizes
    fbs = {name: _fb((2 * v[0] + 3) // 4 * 4, v[1]) for name, v in E.CASES.items()}
    assert fbs["small-tile-64-56"] == 32 and fbs["small-tile-20-240"] == 32 and fbs["40-64"] == 64 and fbs["4-256"] == 64
