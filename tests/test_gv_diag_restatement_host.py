"""Host only: pins tests/gv_diag_restatement.py (one epoch of the GV ascent over diagonal conditional precisions, dense statement
and three-point stencil) and shows that the inputs of tests/test_gpu_gv_diag.py can see a wrong epoch.

  stencil      the tridiagonal form of P y and r equals gv_restatement.gradient_terms(dense=True) -- the reference's statement with
               the matrix W -- to 1e-15 relative, T = 2, 3, 4, 5 among the cases, for both converter kinds; the magnitude the bar is
               fed equals gradient_terms' own with Emag in place of E;
  oracle       iterating the restatement gives oracle/np_oracle.py's trajgv_fvconvert on the expanded cross-diagonal model;
  conditions   every case, at every epoch count n whose step the GPU test checks: both summands >= 0.2 of the step (n >= 1; at
               n = 0 the GV term is zero by eq. (58)), the step >= 1e-5 of max |y|, y finite and within 10 max |y_0|; the arg-max is
               decided with a margin far above its rounding (and takes the prescribed mixture sequence, M = 256 apart);
  sensitivity  every mutant of gv_diag_restatement.MUTANTS misses the unmutated step by >= 100 bars in some element of some checked
               step of every case (the two mutants of the +-2 terms where the utterance has such terms: T >= 3);
  launch rule  the restated rule puts the cases into every form: 5, 4, 3, 2 resident arrays and streamed.

Everything here comes from numpy and the restatements: no number is taken from a run of the kernel."""
import functools

import numpy as np
import pytest

import gv_diag_restatement as gd
import gv_restatement as gr
from gv_restatement import LD
from oracle import np_oracle as npo

IDS = [f"{i}-{c.id}" for i, c in enumerate(gd.ALL_CASES)]
SMALL = [i for i, c in enumerate(gd.ALL_CASES) if c.D * c.T <= 12 * 50 and i < len(gd.CASES)]


@functools.lru_cache(maxsize=None)
def _run(i):
    c = gd.ALL_CASES[i]
    inp = gd.inputs(c)
    _, kept = gd.ascent(inp["pieces"], inp["y0"], max(c.ns) + 1, c.alpha, keep=tuple(c.ns) + (max(c.ns) + 1,))
    return inp, kept


@pytest.mark.parametrize("i", SMALL, ids=[IDS[i] for i in SMALL])
def test_stencil_is_the_dense_statement(i):
    c = gd.ALL_CASES[i]
    inp, kept = _run(i)
    p = inp["pieces"]
    for y in (inp["y0"], kept[max(c.ns)]):
        lik_d, gv_d, mag_d, _ = gr.gradient_terms(p, y, dense=True)
        Py, r = gd.stencil_terms(p, y)
        lik_s = (r - Py) / (2 * c.T)
        scale = float(np.max(np.abs(r)) + np.max(np.abs(Py))) / (2 * c.T)
        assert float(np.max(np.abs(lik_s - lik_d))) <= 1e-15 * scale, c.id
        lik, gv = gd.gradient(p, y)
        assert np.array_equal(lik, lik_s) and float(np.max(np.abs(gv - gv_d))) <= 1e-15 * max(float(np.max(np.abs(gv_d))), 1e-300)
        # P y and r apart: r alone is the dense statement at y = 0
        lik_0 = gr.gradient_terms(p, np.zeros_like(y), dense=True)[0]
        assert float(np.max(np.abs(r / (2 * c.T) - lik_0))) <= 1e-15 * float(np.max(np.abs(r))) / (2 * c.T)
        # the magnitude: gradient_terms' lik_mag of the pieces with Emag as E, and it bounds the one with |E|
        mag_e = gr.gradient_terms(p.with_magnitude_as_E(), y, dense=True)[2]
        mine = gd.lik_magnitude(p, y)
        assert float(np.max(np.abs(mine - mag_e))) <= 1e-15 * float(np.max(mag_e))
        assert np.all(mine >= mag_d * (1 - 1e-15)) and np.all(p.Emag >= np.abs(p.E) * (1 - 1e-15))


def test_short_cases_are_among_the_small_ones():
    assert {2, 3, 4, 5} <= {gd.ALL_CASES[i].T for i in SMALL if gd.ALL_CASES[i].kind == "bdiag"}
    assert {2, 3, 4, 5} <= {gd.ALL_CASES[i].T for i in SMALL if gd.ALL_CASES[i].kind == "dense"}


def test_iterated_restatement_is_the_oracles_ascent_on_the_expanded_model():
    import traj_bdiag_restatement as tb
    c = next(c for c in gd.CASES if (c.kind, c.D, c.T) == ("bdiag", 12, 17))
    inp = gd.inputs(c)
    tj = npo.TrajectoryGMMMap(npo.GMMMap(*tb.expanded_model(*inp["model"])))
    assert np.array_equal(tj.g.predict(inp["X"]), inp["s"])
    mine, _ = gd.ascent(inp["pieces"], inp["y0"], 20, c.alpha)
    want = npo.trajgv_fvconvert(tj, inp["X"], inp["muv"], inp["Sv"], epochs=20, alpha=c.alpha)
    assert np.max(np.abs(mine - want)) < 1e-11 * np.max(np.abs(want))
    assert float(np.max(np.abs(mine - inp["y0"])) / np.max(np.abs(inp["y0"]))) > 1e-4       # ... about an ascent that moves


def _shares(c, p, y):
    lik, gv = gd.gradient(p, y)
    dy = float(np.max(np.abs(lik + gv)))
    return float(np.max(np.abs(gv))) / dy, float(np.max(np.abs(lik))) / dy, c.alpha * dy / float(np.max(np.abs(y)))


@pytest.mark.parametrize("i", range(len(gd.ALL_CASES)), ids=IDS)
def test_input_conditions(i):
    c = gd.ALL_CASES[i]
    inp, kept = _run(i)
    p = inp["pieces"]
    # the arg-max is decided by far more than its rounding: the device and the restatement work on the same mhat
    if c.kind == "bdiag":
        assert np.array_equal(p.mhat, inp["s"])                      # ... and takes the prescribed sequence
        gap, bound = inp["conv"].undecided(inp["X"])
        assert np.all(gap > 1.0) and np.all(gap > 1e6 * bound)
    else:                                                            # (256 mixtures in 8 dimensions overlap: another mixture may win)
        L = np.sort(np.stack([inp["conv"].g.log_weighted(x) for x in inp["X"]]), axis=1)
        assert np.all(L[:, -1] - L[:, -2] > 1e-3), float(np.min(L[:, -1] - L[:, -2]))
        assert c.M == 256 or np.array_equal(p.mhat, inp["s"])
    top = float(np.max(np.abs(inp["y0"])))
    for n, y in kept.items():
        assert np.all(np.isfinite(y.astype(np.float64))) and float(np.max(np.abs(y))) <= 10 * top, n
    for n in c.ns:
        gv, lik, move = _shares(c, p, kept[n])
        print(f"{c.id} alpha={c.alpha:g} scale={c.cov_scale:g} n={n}: max|gv|/max|dy| {gv:.3f}  max|lik|/max|dy| {lik:.3f}  "
              f"max|alpha dy|/max|y| {move:.2e}")
        assert lik >= 0.2 and move >= 1e-5, (n, lik, move)
        assert gv >= 0.2 if n >= 1 else gv < 1e-9, (n, gv)


@pytest.mark.parametrize("i", range(len(gd.ALL_CASES)), ids=IDS)
def test_mutants_miss_the_bar_a_hundredfold(i):
    c = gd.ALL_CASES[i]
    inp, kept = _run(i)
    p = inp["pieces"]
    worst = {m: 0.0 for m in gd.MUTANTS}
    for n in c.ns:
        y = kept[n]
        right = gd.step(p, y, c.alpha)
        bar = gd.step_bar_diag(p, c.alpha, y, right, gr.gv_term(p.pv, p.muv, y)[1])
        for m in gd.MUTANTS:
            worst[m] = max(worst[m], float(np.max(np.abs(gd.step(p, y, c.alpha, m) - right) / bar)))
    print(c.id, {m: f"{v:.1e}" for m, v in worst.items()})
    if c.T == 2:       # no +-2 neighbour at all: these two mutants ARE the epoch
        for m in ("gauss_seidel", "c2_wrong_neighbour"):
            assert worst.pop(m) == 0.0
    assert all(v >= 100.0 for v in worst.values()), {m: v for m, v in worst.items() if v < 100.0}


def test_launch_rule_puts_the_cases_into_every_form():
    forms = {(c.D, c.T): gd.gvd_resident(c.D, c.T) for c in gd.CASES}
    assert set(forms.values()) == {0, 2, 3, 4, 5}, forms
    assert forms[(40, 300)] == 0 and forms[(12, 50)] == 5 and forms[(59, 70)] == 4
    # the edges at D = 12: the last T of a form and the first of the next
    for T, a, b in ((323, 5, 4), (403, 4, 3), (538, 3, 2), (807, 2, 0)):
        assert (gd.gvd_resident(12, T), gd.gvd_resident(12, T + 1)) == (a, b), T
    # vc's default chunks at the headline dimension, D = 40 and 100 frames: four of the five arrays resident
    assert gd.gvd_resident(40, 100) == 4 and gd.gvd_resident(40, 2000) == 0 and gd.gvd_resident(59, 2000) == 0
    # a batch runs in the form of its longest member
    Ts = gd.BATCH_TS
    assert gd.gvd_resident(12, max(Ts)) == 0 and sorted(gd.gvd_resident(12, T) for T in Ts) == [0, 2, 4]
