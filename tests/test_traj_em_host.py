"""CPU: the numpy restatement of the trajectory EM re-estimation (tests/traj_em_restatement.py) against the existing oracle and
against scipy, and the conditions that tests/test_gpu_traj_em.py takes for granted about its inputs -- so that the GPU
test never has to decide whether its inputs are fair."""
import numpy as np
import pytest

import traj_em_restatement as R
from conftest import relerr
from oracle import np_oracle as npo

ALL = list(R.CASES)


def utterances(name):
    (w, mu, sig), Xs = R.case_inputs(name)
    return [(X, r) for X, r in zip(Xs, R.case_reference(name)) if r is not None]


@pytest.mark.parametrize("name", ALL)
def test_iteration_zero_is_the_oracles_conversion(name):
    (w, mu, sig), Xs = R.case_inputs(name)
    tj = npo.TrajectoryGMMMap(npo.GMMMap(w, mu, sig))
    for X, r in utterances(name):
        assert np.array_equal(r["ys"][0], tj.fvconvert(X)[0])
        assert len(r["ys"]) == len(r["L"]) == len(r["gamma"]) == len(r["gap"]) == R.NITER + 1
        assert np.allclose(r["gamma"][0].sum(axis=0), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ALL)
def test_objective_never_falls(name):
    """EM's guarantee; the slack is summation rounding of sum_t lse_t (worst step seen on these inputs: -4e-16 relative)."""
    for X, r in utterances(name):
        L = np.array(r["L"])
        assert np.all(np.diff(L) >= -1e-10 * np.abs(L[:-1])), L


@pytest.mark.parametrize("name", ["stencil-12", "native-20", "padded-7", "zero-weight-12"])
def test_objective_against_scipy(name):
    """L(y) = sum_t log sum_m pi_{m,t} N((W y)_t; E_{m,t}, Q_m^-1), each density from scipy.stats.multivariate_normal.  The
    synthetic covariances are exactly symmetric, so Q_m is symmetric to rounding."""
    from scipy.special import logsumexp
    from scipy.stats import multivariate_normal
    (w, mu, sig), Xs = R.case_inputs(name)
    mdl = R.Model(w, mu, sig)
    for X, r in utterances(name):
        T, D2 = X.shape
        D = D2 // 2
        W = npo.constructW(D, T)
        logpi, E = mdl.log_prior(X), mdl.means(X)
        for k in (0, 1, R.NITER):
            Y = (W @ r["ys"][k].ravel()).reshape(T, D2)
            tot = 0.0
            for t in range(T):
                terms = []
                for m in range(mdl.g.M):
                    if not w[m] > 0.0:
                        continue
                    cov = np.linalg.inv(0.5 * (mdl.Q[m] + mdl.Q[m].T))
                    terms.append(logpi[t, m] + multivariate_normal(E[m, t], 0.5 * (cov + cov.T)).logpdf(Y[t]))
                tot += logsumexp(terms)
            assert abs(tot - r["L"][k]) <= 1e-10 * abs(tot), (k, tot, r["L"][k])


@pytest.mark.parametrize("name", R.OVERLAP)
def test_overlapping_inputs_blend_every_frame(name):
    """What the GPU file's parity and likelihood assertions need from an overlapping model: every frame is mixed at every E-step
    (so no frame sits at the pure / mixed decision), the objective rises strictly in the first iteration and y really moves (5 .. 96 % of max |y|)."""
    for X, r in utterances(name):
        for g in r["gamma"]:
            assert np.all(1.0 - g.max(axis=0) >= 2.0 ** -40)
        L = r["L"]
        assert L[1] - L[0] > 5e-8 * abs(L[0])                         # (the GPU file's slack for rounding is 1e-10 |L|)
        assert 0.04 < relerr(r["ys"][1], r["ys"][0]) < 0.97           # measured: 5 .. 96 % of max |y|


@pytest.mark.parametrize("name", R.OVERLAP)
def test_overlapping_inputs_are_well_conditioned(name):
    """A 1e-13 relative perturbation of X moves y^n by at most 1e-12 (measured on these inputs: 0.6 .. 2.1e-13): three orders
    below the GPU parity tolerance of 1e-9."""
    (w, mu, sig), Xs = R.case_inputs(name)
    X, r = max(utterances(name), key=lambda p: len(p[0]))
    rng = np.random.default_rng(1)
    Xp = X * (1.0 + 1e-13 * rng.standard_normal(X.shape))
    rp = R.em_convert(w, mu, sig, Xp, R.NITER)
    for k in (1, 2, R.NITER):
        assert relerr(rp["ys"][k], r["ys"][k]) < 1e-12


@pytest.mark.parametrize("name", R.PEAKED)
def test_peaked_inputs_have_no_mixed_frame(name):
    for X, r in utterances(name):
        for g, gap in zip(r["gamma"], r["gap"]):
            assert np.all(1.0 - g.max(axis=0) < 2.0 ** -53) and gap.min() > 100.0
        assert relerr(r["ys"][R.NITER], r["ys"][0]) < 1e-13


def test_zero_weight_mixture_stays_out():
    (w, mu, sig), Xs = R.case_inputs("zero-weight-12")
    zero = R.CASES["zero-weight-12"][6]
    assert w[zero] == 0.0
    for X, r in utterances("zero-weight-12"):
        for g in r["gamma"]:
            assert np.all(g[zero] == 0.0) and np.all(np.isfinite(g))


def test_fixture_has_pure_and_mixed_frames_in_one_table():
    """The trained model on the golden X: a handful of mixed frames among pure ones at the first E-step, clear decisions
    afterwards, and the rise of the objective that makes the shortcut matter."""
    _, X, r = R.fixture_reference()
    mixed0 = 1.0 - r["gamma"][0].max(axis=0) >= 2.0 ** -53
    assert 1 <= mixed0.sum() <= 20 and mixed0.sum() < len(X)
    assert 0.1 < r["gap"][0][mixed0].min() and r["gap"][0][mixed0].max() < 37.0
    for k in range(1, R.NITER + 1):
        assert r["gap"][k].min() > 40.0
    L = r["L"]
    assert L[0] < -4e5 and L[1] > -6.1e4 and L[2] > L[1]
    mh = [np.argmax(g, axis=0) for g in r["gamma"]]
    assert (mh[R.NITER] != npo.GMMMap(*_).predict(X) - 1).sum() > 30
