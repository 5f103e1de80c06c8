"""Host only: pins tests/gv_penta_restatement.py (one epoch of the GV ascent over three windows, dense statement and five-point
stencil) and shows that the inputs of tests/test_gpu_gv_penta.py can see a wrong epoch.

  stencil      the five-point form of P y and r equals the statement through the explicit W of
               traj_penta_restatement.construct_w and diag(q) to 1e-15 relative, T = 2, 3, 4, 5 among the cases; so does the
               operator form that carries the mutants; the magnitude the bar is fed equals the dense one with Emag in place of E;
  iteration    iterating the stencil equals iterating the dense statement;
  conditions   every case, at every epoch count n whose step the GPU test checks: both summands >= 0.2 of the step (n >= 1; at
               n = 0 the GV term is zero by eq. (58)), the step >= 1e-5 of max |y|, y finite and within 10 max |y_0|; the arg-max
               is decided with a margin far above its rounding and takes the prescribed mixture sequence;
  sensitivity  every mutant of gv_penta_restatement.MUTANTS misses the unmutated step by >= 100 bars in some element of some
               checked step of every case (the mutants of the +-2 terms where the utterance has such terms: T >= 3);
  launch rule  the restated rule puts the cases into every form -- 6, 5, 4, 3, 2 resident arrays and streamed -- and equals
               csrc/traj_band_plan.hpp at the edges (the table tests/c/traj_gvp_check.cpp prints);
  C++          tests/c/traj_gvp_check.cpp: csrc/traj_gv_band_step.hpp run on the CPU over chains against a long-double evaluation, and
               the invariants of the launch rule -- a stand-alone program under ASan + UBSan; nothing is loaded into Python.

Everything here comes from numpy and the restatements: no number is taken from a run of the kernel."""
import functools
import os
import subprocess

import numpy as np
import pytest

import gv_penta_restatement as gp
import gv_restatement as gr
from conftest import ROOT
from gv_restatement import LD

IDS = [f"{i}-{c.id}" for i, c in enumerate(gp.ALL_CASES)]
SMALL = [i for i, c in enumerate(gp.ALL_CASES) if c.D * c.T <= 12 * 50 and i < len(gp.CASES)]


@functools.lru_cache(maxsize=None)
def _run(i):
    c = gp.ALL_CASES[i]
    inp = gp.inputs(c)
    _, kept = gp.ascent(inp["pieces"], inp["y0"], max(c.ns) + 1, c.alpha, keep=tuple(c.ns) + (max(c.ns) + 1,))
    return inp, kept


@pytest.mark.parametrize("i", SMALL, ids=[IDS[i] for i in SMALL])
def test_stencil_is_the_dense_statement(i):
    c = gp.ALL_CASES[i]
    inp, kept = _run(i)
    p = inp["pieces"]
    for y in (inp["y0"], kept[max(c.ns)]):
        lik_d, gv_d, mag_d, _ = gp.gradient_terms(p, y, dense=True)
        Py, r = gp.stencil_terms(p, y)
        lik_s = (r - Py) / (2 * c.T)
        scale = float(np.max(np.abs(r)) + np.max(np.abs(Py))) / (2 * c.T)
        assert float(np.max(np.abs(lik_s - lik_d))) <= 1e-15 * scale, c.id
        lik, gv = gp.gradient(p, y)
        assert np.array_equal(lik, lik_s) and np.array_equal(gv, gr.gv_term(p.pv, p.muv, y)[0]) and np.array_equal(gv, gv_d)
        # the operator form (the one the dense mutants are made in)
        lik_o, _, mag_o, _ = gp.gradient_terms(p, y)
        assert float(np.max(np.abs(lik_o - lik_d))) <= 1e-15 * scale and float(np.max(np.abs(mag_o - mag_d))) <= 1e-15 * float(np.max(mag_d))
        # P y and r apart: r alone is the dense statement at y = 0
        lik_0 = gp.gradient_terms(p, np.zeros_like(y), dense=True)[0]
        assert float(np.max(np.abs(r / (2 * c.T) - lik_0))) <= 1e-15 * float(np.max(np.abs(r))) / (2 * c.T)
        # the magnitude: the dense lik_mag of the pieces with Emag as E, and it bounds the one with |E|
        mag_e = gp.gradient_terms(p.with_magnitude_as_E(), y, dense=True)[2]
        mine = gp.lik_magnitude(p, y)
        assert float(np.max(np.abs(mine - mag_e))) <= 1e-15 * float(np.max(mag_e))
        assert np.all(mine >= mag_d * (1 - 1e-15)) and np.all(p.Emag >= np.abs(p.E) * (1 - 1e-15))


def test_short_cases_are_among_the_small_ones():
    assert {2, 3, 4, 5} <= {gp.ALL_CASES[i].T for i in SMALL}


@pytest.mark.parametrize("T", [2, 3, 4, 5, 17])
def test_iterating_the_stencil_is_iterating_the_dense_statement(T):
    c = next(c for c in gp.CASES if (c.D, c.T) == (12, T))
    inp = gp.inputs(c)
    p = inp["pieces"]
    mine, _ = gp.ascent(p, inp["y0"], 20, c.alpha)
    y = np.asarray(inp["y0"], dtype=LD)
    for _ in range(20):
        lik, gv, _, _ = gp.gradient_terms(p, y, dense=True)
        y = y + LD(c.alpha) * (lik + gv)
    assert float(np.max(np.abs(mine - y))) <= 1e-14 * float(np.max(np.abs(y)))
    assert float(np.max(np.abs(mine - inp["y0"])) / np.max(np.abs(inp["y0"]))) > 1e-4        # ... about an ascent that moves
    # an FP64 ascent (y rounded after every epoch) stays within a few 2^-53 per epoch of it
    y64, _ = gp.ascent(p, inp["y0"], 20, c.alpha, fp64=True)
    assert float(np.max(np.abs(y64 - mine))) <= 20 * 4 * gr.EPS * float(np.max(np.abs(mine)))


def _shares(c, p, y):
    lik, gv = gp.gradient(p, y)
    dy = float(np.max(np.abs(lik + gv)))
    return float(np.max(np.abs(gv))) / dy, float(np.max(np.abs(lik))) / dy, c.alpha * dy / float(np.max(np.abs(y)))


@pytest.mark.parametrize("i", range(len(gp.ALL_CASES)), ids=IDS)
def test_input_conditions(i):
    c = gp.ALL_CASES[i]
    inp, kept = _run(i)
    p = inp["pieces"]
    assert p.D == c.D and p.E.shape == (c.T, 3 * c.D) and np.all(inp["conv"].q > 0)
    # the arg-max is decided by far more than its rounding, and takes the prescribed sequence: device and restatement share mhat
    assert np.array_equal(p.mhat, inp["s"])
    gap, bound = inp["conv"].undecided(inp["X"])
    assert np.all(gap > 1.0) and np.all(gap > 1e6 * bound)
    assert 1.0 <= inp["cond"] < 1e4 and inp["rho"] >= 1.0
    top = float(np.max(np.abs(inp["y0"])))
    for n, y in kept.items():
        assert np.all(np.isfinite(y.astype(np.float64))) and float(np.max(np.abs(y))) <= 10 * top, n
    for n in c.ns:
        gv, lik, move = _shares(c, p, kept[n])
        print(f"{c.id} alpha={c.alpha:g} scale={c.cov_scale:g} n={n}: max|gv|/max|dy| {gv:.3f}  max|lik|/max|dy| {lik:.3f}  "
              f"max|alpha dy|/max|y| {move:.2e}")
        assert lik >= 0.2 and move >= 1e-5, (n, lik, move)
        assert gv >= 0.2 if n >= 1 else gv < 1e-9, (n, gv)


@pytest.mark.parametrize("i", range(len(gp.ALL_CASES)), ids=IDS)
def test_mutants_miss_the_bar_a_hundredfold(i):
    c = gp.ALL_CASES[i]
    inp, kept = _run(i)
    p = inp["pieces"]
    worst = {m: 0.0 for m in gp.MUTANTS}
    for n in c.ns:
        y = kept[n]
        right = gp.step(p, y, c.alpha)
        bar = gp.step_bar(p, c.alpha, y, right, gr.gv_term(p.pv, p.muv, y)[1])
        for m in gp.MUTANTS:
            worst[m] = max(worst[m], float(np.max(np.abs(gp.step(p, y, c.alpha, m) - right) / bar)))
    print(c.id, {m: f"{v:.1e}" for m, v in worst.items()})
    if c.T == 2:       # no +-2 neighbour at all: these two mutants ARE the epoch
        for m in ("c2_wrong_neighbour", "c2_without_pa"):
            assert worst.pop(m) == 0.0
    assert all(v >= 100.0 for v in worst.values()), {m: v for m, v in worst.items() if v < 100.0}


def test_launch_rule_puts_the_cases_into_every_form():
    forms = {(c.D, c.T): gp.gvp_resident(c.D, c.T) for c in gp.CASES}
    assert set(forms.values()) == {0, 2, 3, 4, 5, 6}, forms
    assert forms[(40, 300)] == 0 and forms[(12, 50)] == 6 and forms[(12, 2)] == 6
    # the edges at D = 12: the last T of a form and the first of the next
    edges = ((269, 6, 5), (323, 5, 4), (403, 4, 3), (538, 3, 2), (807, 2, 0))
    for T, a, b in edges:
        assert (gp.gvp_resident(12, T), gp.gvp_resident(12, T + 1)) == (a, b), T
    assert set(gp.EDGE_TS) == {T for T, _, _ in edges} | {T + 1 for T, _, _ in edges}
    # vc's default chunks at the headline dimension, D = 40 and 100 frames: four of the six arrays resident
    assert gp.gvp_resident(40, 100) == 4 and gp.gvp_resident(40, 2000) == 0
    # a batch runs in the form of its longest member
    Ts = gp.BATCH_TS
    assert gp.gvp_resident(12, max(Ts)) == 0 and sorted(gp.gvp_resident(12, T) for T in Ts) == [0, 2, 5]
    for ns in (gp.N_FULL, gp.N_SHORT):      # both parities of the Jacobi buffers among n and n + 1
        assert {n % 2 for n in ns} | {(n + 1) % 2 for n in ns} == {0, 1}
    assert gp.gvp_ws_doubles(1000, 40, True) == 200000 and gp.gvp_ws_doubles(1000, 40, False) == 80000


def test_step_header_and_launch_rule_under_asan_ubsan():
    out = os.path.join(ROOT, "oracle", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "traj_gvp_check_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "traj_gvp_check.cpp"),
           "-fsanitize=address,undefined", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print("\n".join(line for line in p.stdout.splitlines() if not line.startswith("resident")))
    assert p.returncode == 0 and "traj_gvp_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    chains = [line.split() for line in p.stdout.splitlines() if line.startswith("chain T ")]
    assert {int(c[2]) for c in chains} == {2, 3, 4, 5, 50, 2000}
    chains2 = [line.split() for line in p.stdout.splitlines() if line.startswith("two-window chain T ")]     # gvd_epoch_step
    assert {int(c[3]) for c in chains2} == {2, 3, 4, 5, 50, 2000}
    # the rule equals its Python restatement
    table = [line.split() for line in p.stdout.splitlines() if line.startswith("resident D ")]
    assert len(table) == 7 * 16 and {(12, T) for T in gp.EDGE_TS} <= {(int(t[2]), int(t[4])) for t in table}
    for t in table:
        assert gp.gvp_resident(int(t[2]), int(t[4])) == int(t[6]), t


def test_argument_errors_before_a_device_is_touched():
    import ctypes as C
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import _lib
    assert "vcmi_trajgv_create_bdiag" in _lib.SIGNATURES
    assert issubclass(vc.BlockDiagTrajectoryGVGMMMap, vc.DiagTrajectoryGVGMMMap)
    own = {k for k in vars(vc.BlockDiagTrajectoryGVGMMMap) if not k.startswith("__")} | {"__init__"}
    assert own == {"_create", "__init__"}
    for t in (None, object(), "converter", 3):
        with pytest.raises(TypeError, match="BlockDiagTrajectoryGMMMap"):
            vc.BlockDiagTrajectoryGVGMMMap(t, np.ones(3), np.eye(3))
    h = C.c_void_p()
    x = np.ones(3)
    assert _lib.lib.vcmi_trajgv_create_bdiag(None, _lib.dptr(x), _lib.dptr(x), C.byref(h)) != 0 and not h
