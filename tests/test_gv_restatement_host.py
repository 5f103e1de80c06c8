"""Host only: pins tests/gv_restatement.py (one epoch of the GV ascent in long double, the two gradient summands apart) and shows
that the inputs of tests/test_gpu_gv_steps.py can see a wrong epoch.

  parity       iterating the restatement gives np_oracle.trajgv_fvconvert and crosscheck.gv_ascent_dense; the stencil and the
               dense W agree; the gv summand is (T-1)/T times the gradient of log N(var_1(y); mu_v, Sigma_vv) at a point with
               var_1(y) != mu_v (crosscheck.check_gvgrad_is_the_gv_likelihood_gradient, 50-digit central differences);
  conditions   every case of gv_restatement.ALL_CASES, at every epoch count n whose step n -> n + 1 the GPU test checks:
               max |alpha gv| >= 0.2 max |alpha dy| (n >= 1: at n = 0 the term is zero by eq. (58), which the GPU test asserts as
               such), max |alpha lik| >= 0.2 max |alpha dy|, max |alpha dy| >= 1e-5 max |y|, y finite and within 10 max |y_0|;
  sensitivity  every mutant of gv_restatement.MUTANTS misses the unmutated step by >= 100 step_bar in some element of some
               checked step of every case.

Everything here comes from the oracle and the restatement: no number is taken from a run of the kernels."""
import functools

import numpy as np
import pytest

import gv_restatement as gr
from oracle import crosscheck as cc, np_oracle as npo

CASE_IDS = [f"{i}-{c.id}" for i, c in enumerate(gr.ALL_CASES)]


@functools.lru_cache(maxsize=None)
def _run(i):
    """(inputs, y_0, {n: y_n}) of ALL_CASES[i] -- the restatement iterated from the oracle's eq. (58) start"""
    c = gr.ALL_CASES[i]
    inp = gr.inputs(c)
    y0 = npo.variance_scaling(gr.plain_trajectory(inp["tj"], inp["pieces"], inp["X"]), inp["muv"])
    _, kept = gr.ascent(inp["pieces"], y0, max(c.ns) + 1, c.alpha, keep=c.ns + (max(c.ns) + 1,))
    return inp, y0, kept


def test_iterated_restatement_is_the_oracles_ascent():
    c = gr.Case(12, 4, "cycle", 17, 0.1)
    inp = gr.inputs(c)
    w, mu, sig = inp["model"]
    p, X, muv, Sv = inp["pieces"], inp["X"], inp["muv"], inp["Sv"]
    y0, _ = gr.initial(inp["tj"], X, muv)
    mine, _ = gr.ascent(p, y0, 20, c.alpha)
    want = npo.trajgv_fvconvert(inp["tj"], X, muv, Sv, epochs=20, alpha=c.alpha)
    assert np.max(np.abs(mine - want)) < 1e-13 * np.max(np.abs(want))
    dense, first = cc.gv_ascent_dense(w, mu, sig, X, muv, Sv, 20, c.alpha)
    assert np.max(np.abs(mine - dense)) < 1e-11 * np.max(np.abs(dense))      # (another solver for the start: cond(P) 2^-53)
    moved = float(np.max(np.abs(mine - y0)) / np.max(np.abs(y0)))
    assert moved > 1e-3, moved                                                # the agreement above is about an ascent that moves
    # the first gradient of the dense evaluation is lik alone (gv = 0 at the start), and the two forms of W agree
    lik, gv, lik_mag, gv_mag = gr.gradient_terms(p, y0)
    assert np.max(np.abs(lik + gv - first)) < 1e-11 * np.max(np.abs(first))
    y7 = gr.ascent(p, y0, 7, c.alpha)[0]
    a, b = gr.gradient_terms(p, y7), gr.gradient_terms(p, y7, dense=True)
    for u, v in zip(a, b):
        assert np.max(np.abs(u - v)) <= 64 * 2.0 ** -63 * np.max(a[2] + a[3])
    assert np.all(a[2] >= np.abs(a[0])) and np.all(a[3] >= np.abs(a[1]))     # a magnitude bounds its term


def test_gv_summand_is_the_gv_likelihood_gradient():
    rng = np.random.default_rng(4)
    T, D = 5, 3
    y = rng.standard_normal((T, D)) * np.array([1.0, 0.5, 2.0]) + 3.0
    muv = np.array([0.8, 1.1, 0.6])
    Sv = np.diag([0.2, 0.1, 0.3]) + 0.02                  # symmetric: the log-density knows only the symmetric part
    assert np.max(np.abs(y.var(axis=0, ddof=1) / muv - 1.0)) > 0.2       # var_1(y) != mu_v: the term is not zero here

    def fn(pv, muv_, y_):
        return gr.gv_term(pv, muv_, y_)[0].astype(np.float64)

    assert np.max(np.abs(fn(np.linalg.inv(Sv), muv, y))) > 0.1
    cc.check_gvgrad_is_the_gv_likelihood_gradient(y, muv, Sv, fn, rel=1e-12)
    assert np.max(np.abs(fn(np.linalg.inv(Sv), muv, y) - npo.gvgrad(np.linalg.inv(Sv), muv, y))) < 1e-14


def _shares(c, p, y):
    lik, gv, _, _ = gr.gradient_terms(p, y)
    dy = float(np.max(np.abs(lik + gv)))
    return float(np.max(np.abs(gv))) / dy, float(np.max(np.abs(lik))) / dy, c.alpha * dy / float(np.max(np.abs(y)))


@pytest.mark.parametrize("i", range(len(gr.ALL_CASES)), ids=CASE_IDS)
def test_input_conditions(i):
    c = gr.ALL_CASES[i]
    inp, y0, kept = _run(i)
    assert np.array_equal(inp["pieces"].mhat, inp["s"])              # the oracle's arg-max takes the prescribed sequence
    top = float(np.max(np.abs(y0)))
    for n, y in kept.items():
        assert np.all(np.isfinite(y.astype(np.float64))) and float(np.max(np.abs(y))) <= 10 * top, n
    for n in c.ns:
        gv, lik, move = _shares(c, inp["pieces"], kept[n])
        print(f"{c.id} alpha={c.alpha:g} scale={c.cov_scale:g} n={n}: max|gv|/max|dy| {gv:.3f}  max|lik|/max|dy| {lik:.3f}  "
              f"max|alpha dy|/max|y| {move:.2e}")
        assert lik >= 0.2 and move >= 1e-5, (n, lik, move)
        assert gv >= 0.2 if n >= 1 else gv < 1e-9, (n, gv)


def test_fixture_model_setting_meets_the_conditions(fixture_model):
    """the second converter of tests/test_gpu_gv.py::test_fixture_model_gv (the reference's trained model): both terms are
    >= 0.2 of the step at n = 7 and at the last step, the step >= 1e-5 of y, y bounded"""
    from conftest import load_golden
    z = load_golden("trajectory_fixture_model.npz")
    tj = npo.TrajectoryGMMMap(npo.GMMMap(*fixture_model))
    rng = np.random.default_rng(0)                         # _gv_stats of tests/test_gpu_gv.py
    muv = z["Y"].var(axis=0, ddof=1) * 1.3
    A = rng.standard_normal((20, 20))
    Sv = (A @ A.T / 20 * np.mean(muv) ** 2 * 0.1 + np.diag(muv ** 2 * 0.05)) * gr.FIXTURE_COV_SCALE
    p = gr.Pieces(tj, z["X"], muv, Sv)
    y0 = npo.variance_scaling(z["Y"], muv)
    ns = (7, gr.FIXTURE_EPOCHS - 1)
    yN, kept = gr.ascent(p, y0, gr.FIXTURE_EPOCHS, gr.FIXTURE_ALPHA, keep=ns)
    assert float(np.max(np.abs(yN))) <= 10 * float(np.max(np.abs(y0)))
    assert float(np.max(np.abs(yN - y0))) > 1e-3 * float(np.max(np.abs(y0)))
    for n in ns:
        gv, lik, move = _shares(gr.Case(20, 32, "fixture", 100, gr.FIXTURE_ALPHA), p, kept[n])
        print(f"fixture model n={n}: gv {gv:.3f} lik {lik:.3f} step {move:.2e}")
        assert gv >= 0.2 and lik >= 0.2 and move >= 1e-5


def test_a_tile_of_the_mixed_case_holds_three_mixtures():
    c = gr.GV2_CASES[-1]
    s = gr.inputs(c)["s"]
    assert (c.D, c.M) == (20, 6) and min(len(set(s[t:t + 16].tolist())) for t in range(0, c.T, 16)) >= 3


@pytest.mark.parametrize("i", range(len(gr.ALL_CASES)), ids=CASE_IDS)
def test_mutants_miss_the_bar_a_hundredfold(i):
    c = gr.ALL_CASES[i]
    inp, _, kept = _run(i)
    p = inp["pieces"]
    worst = {m: 0.0 for m in gr.MUTANTS}
    for n in c.ns:
        y = kept[n]
        lik, gv, lik_mag, gv_mag = gr.gradient_terms(p, y)
        bar = gr.step_bar(c.D, c.T, c.alpha, y, y + c.alpha * (lik + gv), lik_mag, gv_mag)
        for m in gr.MUTANTS:
            ml, mg, _, _ = gr.gradient_terms(p, y, m, mags=False)
            worst[m] = max(worst[m], float(np.max(np.abs(c.alpha * ((ml + mg) - (lik + gv))) / bar)))
    print(c.id, {m: f"{v:.1e}" for m, v in worst.items()})
    assert all(v >= 100.0 for v in worst.values()), {m: v for m, v in worst.items() if v < 100.0}
