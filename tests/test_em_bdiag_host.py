"""CPU: the cross-diagonal ("block_diag") restatement (tests/em_bdiag_restatement.py) that tests/test_gpu_em_bdiag.py judges
the device by, proved on the host: the float64 M-step lies inside the derived bounds; the centred numpy E-step and the C oracle's
full-covariance E-step on the expanded model -- the two references -- agree with each other, also where an expanded form
would cancel; the layouts of expand_block_diag and of the packed statistics; train_gmm's argument errors, which are raised
before any device call."""
import numpy as np
import pytest

import em_bdiag_restatement as br
from em_restatement import LD
from test_gpu_estep_adversarial import per_mixture_err


@pytest.mark.parametrize("Dj,M,scale", br.MSTEP_BDIAG_SHAPES)
@pytest.mark.parametrize("min_covar", [1e-7, 0.0])
def test_float64_mstep_bdiag_lies_inside_the_bounds(Dj, M, scale, min_covar):
    import voiceconversion_jl_amd as vc
    S0, S1, S2, Sxy = br.mstep_bdiag_case(2000 + Dj + M, Dj, M, scale)
    ref = br.mstep_bdiag(S0, S1, S2, Sxy, min_covar)
    bounds = br.mstep_bdiag_bounds(S0, S1, S2, Sxy, min_covar, ref)
    got = vc.mstep_bdiag(S0, S1, S2, Sxy, min_covar)
    assert got[2].shape == (Dj + Dj // 2, M)
    for name, g, r, b in zip(("w", "mu", "covars"), got, ref, bounds):
        assert g.shape == r.shape == b.shape
        excess = np.max(np.abs(np.asarray(g, dtype=LD) - r) / b)
        print(f"({Dj},{M},{scale:g}) min_covar {min_covar:g}: {name} uses {float(excess):.3f} of its bound")
        assert excess <= 1, (name, float(excess))
    # the bounds are not vacuous: where nothing cancels (scale 1) the cross-covariances keep 12 digits of the pair's scale
    D = Dj // 2
    if scale == 1.0:
        assert np.all(bounds[2][Dj:] <= 1e-12 * np.sqrt(ref[2][:D] * ref[2][D:Dj]))
    # every case stays positive definite by more than the bounds (the GPU test runs min_covar = 0 on that ground)
    assert np.all(br.pairs_valid(np.vstack([ref[2][:Dj] - bounds[2][:Dj], np.abs(ref[2][Dj:]) + bounds[2][Dj:]])))


def test_restatement_empty_mixture():
    """An empty mixture: w = eps, mu = 0, var = min_covar, c = 0 -- exactly, in longdouble as in float64."""
    import voiceconversion_jl_amd as vc
    S0 = np.array([3.0, 0.0])
    S1 = np.array([[6.0, 0.0], [3.0, 0.0]])
    S2 = np.array([[15.0, 0.0], [6.0, 0.0]])
    Sxy = np.array([[7.5, 0.0]])
    for f in (br.mstep_bdiag, vc.mstep_bdiag):
        w, mu, cov = f(S0, S1, S2, Sxy, 1e-3)
        assert float(w[1]) == np.finfo(np.float64).eps and np.all(mu[:, 1] == 0) and np.all(cov[:2, 1] == LD(1e-3)) and cov[2, 1] == 0
        assert abs(float(cov[2, 0]) - (2.5 - 2.0)) < 1e-13 and abs(float(cov[1, 0]) - (1.0 + 1e-3)) < 1e-13


def test_pack_bdiag_stats_is_the_layout_unpack_bdiag_stats_reads():
    import voiceconversion_jl_amd as vc
    S0, S1, S2, Sxy = br.mstep_bdiag_case(5, 6, 4, 1.0)
    p = br.pack_bdiag_stats(S0, S1, S2, Sxy, -7.5)
    assert p.shape == (4 * (1 + 2 * 6 + 3) + 1,)
    u0, u1, u2, uxy, ll = vc.unpack_bdiag_stats(p, 6, 4)
    assert np.array_equal(u0, S0) and np.array_equal(u1, S1) and np.array_equal(u2, S2) and np.array_equal(uxy, Sxy) and ll == -7.5
    # S0, S1 and S2 sit where the diagonal statistics sit
    d0, d1, d2, _ = vc.unpack_stats(p, 6, 4)
    assert np.array_equal(d0, S0) and np.array_equal(d1, S1) and np.array_equal(d2, S2)


def test_expand_block_diag():
    import voiceconversion_jl_amd as vc
    cov = np.arange(1.0, 25.0).reshape(6, 4)                            # Dj = 4, D = 2, M = 4
    s = vc.expand_block_diag(cov)
    assert s.shape == (4, 4, 4) and s.flags.f_contiguous and s.dtype == np.float64
    for m in range(4):
        want = np.diag(cov[:4, m])
        want[0, 2] = want[2, 0] = cov[4, m]
        want[1, 3] = want[3, 1] = cov[5, m]
        assert np.array_equal(s[:, :, m], want)
    assert np.array_equal(s, br.expand(cov))
    assert vc.expand_block_diag(np.array([[2.0], [3.0], [1.0]])).tolist() == [[[2.0], [1.0]], [[1.0], [3.0]]]
    for bad in (np.ones(3), np.ones((4, 2)), np.ones((3, 2, 2))):
        with pytest.raises(vc.DimensionMismatch):
            vc.expand_block_diag(bad)
    # a diagonal fit as a starting point
    var = np.arange(1.0, 9.0).reshape(4, 2)
    assert np.array_equal(vc.expand_block_diag(np.vstack([var, np.zeros((2, 2))])), vc.expand_diag(var))


def test_train_gmm_block_diag_argument_errors_come_before_any_device_call():
    """On a machine without a GPU a device call would fail with another exception type: X never leaves the host."""
    import voiceconversion_jl_amd as vc
    X = np.zeros((4, 10))
    for bad in ("tied", "spherical", None):
        with pytest.raises(ValueError, match="covariance_type") as e:
            vc.train_gmm(X, n_components=2, covariance_type=bad)
        assert all(f"'{n}'" in str(e.value) for n in ("full", "diag", "block_diag"))
    with pytest.raises(vc.DimensionMismatch, match="even"):
        vc.train_gmm(np.zeros((5, 10)), n_components=2, covariance_type="block_diag")
    full = (np.full(2, 0.5), np.zeros((4, 2)), np.repeat(np.eye(4)[:, :, None], 2, axis=2))
    diag = (np.full(2, 0.5), np.zeros((4, 2)), np.ones((4, 2)))
    for refine in (full, diag):
        with pytest.raises(vc.DimensionMismatch, match="block_diag"):
            vc.train_gmm(X, n_components=2, covariance_type="block_diag", refine=refine)


@pytest.mark.parametrize("Dj,M,N", br.ESTEP_BDIAG_SHAPES + [(16, 4, n) for n in br.ESTEP_BDIAG_NS])
def test_the_two_estep_references_agree(Dj, M, N):
    """The centred numpy E-step in float64 against the C oracle's full-covariance E-step (Cholesky of the expanded model):
    1e-11 per mixture, log-likelihood 1e-11 relative."""
    w, mu, cov, X = br.estep_case(Dj, M, N)
    assert np.all(br.pairs_valid(cov)) and X.shape == (N, Dj)
    ref = br.estep_oracle(Dj, M, N)
    got = br.estep_bdiag(X, w, mu, cov)
    e = per_mixture_err(got[:4], ref[:4])
    print(f"({Dj},{M},{N}): numpy against the oracle {e.max():.2e}, loglik {abs(got[4] - ref[4]) / abs(ref[4]):.2e}")
    assert e.max() <= 1e-11, e
    assert abs(got[4] - ref[4]) <= 1e-11 * abs(ref[4])
    if M > 1 and N >= 100:             # the mixtures share frames: responsibilities strictly between 0 and 1 are the rule
        G = np.exp(_logdens(X, w, mu, cov))
        assert np.mean(np.sort(G, axis=1)[:, -2] > 1e-3) > 0.25


def _logdens(X, w, mu, cov):
    """normalised log-responsibilities (N,M) of the model, float64"""
    Dj, D = X.shape[1], X.shape[1] // 2
    L = np.empty((len(X), len(w)))
    for m in range(len(w)):
        vx, vy, c = cov[:D, m], cov[D:Dj, m], cov[Dj:, m]
        det = vx * vy - c * c
        dx, dy = X[:, :D] - mu[:D, m], X[:, D:] - mu[D:, m]
        L[:, m] = np.log(w[m]) - 0.5 * (np.log(det).sum() + ((vy * dx * dx - 2 * c * dx * dy + vx * dy * dy) / det).sum(axis=1))
    return L - np.logaddexp.reduce(L, axis=1)[:, None]


def test_the_oracle_holds_on_the_cancellation_case():
    """Variances 1e-6, |mu| ~ 10, pair correlations +-(1 - 1e-6), two mixtures that differ in their weights only: the C oracle
    against the longdouble restatement at 1e-9 (the bar the device meets on this case), and gamma is the ratio of the weights."""
    from oracle import c_oracle as co
    w, mu, cov, X = br.cancellation_case()
    ref = br.estep_bdiag(X, w, mu, cov, dtype=LD)
    assert abs(float(ref[0][0]) - 0.3 * len(X)) < 1e-9 * len(X) and abs(float(ref[0][1]) - 0.7 * len(X)) < 1e-9 * len(X)
    got = br.full_to_bdiag(*br.oracle_estep_full(co, X, w, mu, cov))
    e = per_mixture_err(got[:4], tuple(np.asarray(r, dtype=np.float64) for r in ref[:4]))
    print(f"oracle against longdouble on the cancellation case: {e.max():.2e}, loglik {abs(got[4] - float(ref[4])) / abs(float(ref[4])):.2e}")
    assert e.max() <= 1e-9, e
    assert abs(got[4] - float(ref[4])) <= 1e-9 * abs(float(ref[4]))
