"""CPU: what tests/test_gpu_traj_em_terms.py takes for granted -- the "half" inputs (pure and mixed frames side by side), the
decision-line inputs, the longdouble terms of one pass and their bounds (tests/traj_em_restatement.py: HALF, LINE, estep_terms,
estep_bounds, check_pass) -- so that the GPU file never has to decide whether its inputs or its checker are fair.  The checker is
tried here on a float64 numpy pass (float_pass), which it must accept, on nine passes that are wrong in one place each, which
it must reject a hundredfold, and on passes with a single NaN in one result, which it must reject although a NaN ratio compares
false with every bound."""
import numpy as np
import pytest

import traj_em_restatement as R
from conftest import relerr

HALF = list(R.HALF)
OLD = ["native-20", "padded-13", "cfg5-40", "big-48", "valu-52"]           # the existing cases the GPU file runs the hook on
LONG = 63                                                                  # "the longer utterances": from here on


def passes(name):
    """-> model, [(X, y, tag)]: every pass the GPU file checks for the case"""
    if name in R.LINE:
        model, X, y, _ = R.line_inputs(name)
        return model, [(X, y, name)]
    if name in R.HALF:
        model, Xs, _ = R.half_inputs(name)
        refs = R.half_reference(name)
    else:
        model, Xs = R.case_inputs(name)
        refs = R.case_reference(name)
    return model, [(X, r["ys"][j], f"{name} T={len(X)} y^{j}") for X, r in zip(Xs, refs) if r is not None for j in (0, 2)]


@pytest.mark.parametrize("name", HALF)
def test_half_inputs_hold_pure_and_mixed_frames_side_by_side(name):
    """At every E-step of the restatement every frame is clearly one or the other (best-to-second gap below 30 or above 45
    nats); the longer utterances are at least 40 % of each and every 16-frame tile of theirs holds both (the window of
    all-mixed frames of "gap" aside); the first iteration moves y by at least 4 % of max |y|; the models have cond <= 2."""
    D, Mo, Mi, Ts, _, special = R.HALF[name]
    model, Xs, Zs = R.half_inputs(name)
    assert R.term_model(model).cond <= 2.0 + 1e-9
    for X, z, r in zip(Xs, Zs, R.half_reference(name)):
        T = len(X)
        for gap in r["gap"]:
            assert np.all((gap < 30.0) | (gap > 45.0)), gap[(gap >= 30.0) & (gap <= 45.0)]
            pure = gap > 45.0
            assert np.array_equal(pure, z >= Mo)                          # the labels decide, at every E-step
            if T >= LONG:
                assert 0.4 * T <= pure.sum() <= 0.6 * T, (T, pure.sum())
                for t0 in range(0, T - 15, 16):
                    if special == "gap" and 64 <= t0 < 128:
                        assert not pure[t0:t0 + 16].any()
                    else:
                        assert pure[t0:t0 + 16].any() and not pure[t0:t0 + 16].all(), t0
        moved = relerr(r["ys"][1], r["ys"][0])
        print(f"{name} T={T}: first iteration moves y by {moved:.3f} of max |y|")
        assert moved >= 0.04
        if special == "edge" and T > 1024:
            assert z[1023] < Mo and z[1024] < Mo                          # mixed frames on both sides of the scan's chunk edge
        if special == "late":
            last = Mo + Mi - 1
            assert not np.any(z[:64] == last) and np.any(z[64:] == last)
            g0 = r["gamma"][0]
            assert np.all(g0[last, :64] == 0.0)                            # exactly: need[] of the first workgroup stays 0
        if special == "gap":
            assert np.all(r["gamma"][0][Mo:, 64:128] == 0.0)              # the whole isolated group is skipped there


@pytest.mark.parametrize("name", HALF)
def test_half_inputs_are_well_conditioned(name):
    """tests/test_traj_em_host.py::test_overlapping_inputs_are_well_conditioned on the new cases: a 1e-13 relative perturbation of
    X moves y^n of the longest utterance by less than 1e-11 of max |y| (measured: 0.6 .. 2.3e-12) -- two orders below the GPU
    parity tolerance of 1e-9.  The all-mixed cases stay below 1e-12; here the isolated source means sit 6 (k + 1) from the origin
    in every coordinate, so a RELATIVE perturbation of X is up to 6 Mi + 3 ~ 20 times larger against x - mux, which is what y
    depends on: ten times the all-mixed threshold.  The pure frames' decisions are more than 45 nats from the line."""
    (w, mu, sig), Xs, _ = R.half_inputs(name)
    k = max(range(len(Xs)), key=lambda i: len(Xs[i]))
    X, r = Xs[k], R.half_reference(name)[k]
    rng = np.random.default_rng(1)
    rp = R.em_convert(w, mu, sig, X * (1.0 + 1e-13 * rng.standard_normal(X.shape)), R.NITER)
    moved = [relerr(rp["ys"][n], r["ys"][n]) for n in (1, 2, R.NITER)]
    print(f"{name}: a 1e-13 perturbation of X moves y^1, y^2, y^4 by", " ".join(f"{m:.2e}" for m in moved))
    assert max(moved) < 1e-11


@pytest.mark.parametrize("name", HALF + OLD)
def test_no_undecided_frame_outside_the_decision_line_cases(name):
    model, items = passes(name)
    for X, y, tag in items:
        b = R.estep_bounds(model, X, y)
        assert np.all(b["must_mix"] | b["must_pure"]), tag
        assert not np.any(b["must_mix"] & b["must_pure"])


@pytest.mark.parametrize("name", list(R.LINE))
def test_decision_line_inputs(name):
    """The bisection lands on its levels to 1e-12 in log r; the frames inside the undecided band are targets with a level in
    [-37.5, -30], every other frame -- the targets at -40 and -45 included -- is decided by the restatement alone."""
    model, X, y, lev = R.line_inputs(name)
    b = R.estep_bounds(model, X, y)
    tg = ~np.isnan(lev)
    assert tg.sum() == len(range(1, len(X), 4)) and set(lev[tg]) == set(R.LINE_LEVELS)
    assert np.max(np.abs(np.log(np.asarray(b["ref"]["r"][tg], dtype=np.float64)) - lev[tg])) < 1e-12
    und = ~b["must_mix"] & ~b["must_pure"]
    assert np.all((lev[und] >= -37.5) & (lev[und] <= -30.0))               # (nan compares false: a non-target fails here)
    assert np.all(b["must_pure"][tg & (lev <= -40.0)]) and np.all((b["must_mix"] | b["must_pure"])[~tg])
    print(f"{name}: {int(und.sum())} of {int(tg.sum())} targets are undecided; |l_best| of the targets "
          f"{np.abs(np.asarray(b['ref']['ell'], dtype=np.float64)).min(axis=1)[tg].min():.0f} .. "
          f"{np.abs(np.asarray(b['ref']['ell'], dtype=np.float64)).min(axis=1)[tg].max():.0f}")


@pytest.mark.parametrize("name", HALF + OLD + list(R.LINE))
def test_longdouble_terms_agree_with_the_float64_restatement(name):
    """estep_terms against Model.estep (written from np_oracle, float64, sharing no code with it), and check_pass accepts the
    float64 pass: every ratio is far below 1 (printed)."""
    model, items = passes(name)
    mdl = R.Model(*model)
    for X, y, tag in items:
        ref = R.estep_terms(model, X, y)
        ell, lse, gamma, L = mdl.estep(X, np.asarray(y))
        f = lambda a: np.asarray(a, dtype=np.float64)                      # noqa: E731
        assert np.all(np.abs(ell.T - f(ref["ell"])) <= 1e-9 * (1.0 + np.abs(ell.T)))
        assert np.all(np.abs(lse - f(ref["lse"])) <= 1e-9 * (1.0 + np.abs(lse)))
        assert np.all(np.abs(gamma.T - f(ref["gamma"])) <= 1e-9)
        assert abs(L - float(ref["lse"].sum())) <= 1e-10 * abs(L)
        ratios, problems = R.check_pass(R.estep_bounds(model, X, y), R.float_pass(model, X, y))
        print(tag, "float64 pass, error / bound:", " ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
        assert R.accepted(ratios, problems), (tag, ratios, problems)


# the cases each mutant is tried on: mixed and pure frames, two workgroups, a mixture range with small weights, the line
MUTANT_CASES = ["half-20", "half-12-m33", "line-130"]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_a_pass_that_is_wrong_in_one_place_misses_a_bound_a_hundredfold(mutant):
    """wrap: the missing neighbour at t = 0 / T-1 not dropped; weight: delta weight 1 for 1/2; no-c: c_m omitted; unnormalised: log
    pi without its normalisation; swap-gamma: gamma of two adjacent frames swapped; shift-workgroup: the frames from t = 64 on
    read one frame further; drop-small: mixtures with gamma < 1e-8 left out of gbar; blend-k+1: blended matrix k written to
    k + 1; pure-m+1: a pure frame indexing the next mixture."""
    worst, where = 0.0, None
    for name in MUTANT_CASES:
        model, items = passes(name)
        for X, y, tag in items:
            ratios, problems = R.check_pass(R.estep_bounds(model, X, y), R.float_pass(model, X, y, mutant))
            k = max(ratios, key=ratios.get)
            if ratios[k] > worst:
                worst, where = ratios[k], f"{k} of {tag}" + (f" ({problems[0]})" if problems else "")
    print(f"mutant {mutant}: misses its bound {worst:.3g}-fold at {where}")
    assert worst >= 100.0


@pytest.mark.parametrize("mutant", R.NAN_MUTANTS)
def test_a_single_nan_is_rejected(mutant):
    """One NaN in lse, in a mixed frame's gamma, in gbar or in a blended matrix: its ratio is NaN, which compares false both
    ways, so the verdict must not rest on a maximum -- check_pass names the value as a problem and accepted() refuses a ratio
    that is not finite."""
    for name in MUTANT_CASES:
        model, items = passes(name)
        X, y, tag = items[0]
        ratios, problems = R.check_pass(R.estep_bounds(model, X, y), R.float_pass(model, X, y, mutant))
        key = {"nan-table": "Qbar"}.get(mutant, mutant[4:])
        print(f"mutant {mutant} on {tag}: ratio {key} = {ratios[key]}; {problems}")
        assert np.isnan(ratios[key]) and any("not finite" in p for p in problems)
        assert not R.accepted(ratios, problems) and not R.accepted(ratios, [])
