"""CPU: the diagonal M-step restatement and its error bounds (tests/em_diag_restatement.py) that tests/test_gpu_em_diag.py
judges the device by, proved against plain float64 numpy; expand_diag; train_gmm's argument errors, which are raised
before any device call; and the recovery input of the GPU suite, checked once with a numpy EM."""
import numpy as np
import pytest

import em_diag_restatement as dr
from em_restatement import LD


@pytest.mark.parametrize("Dj,M,scale", dr.MSTEP_DIAG_SHAPES)
@pytest.mark.parametrize("min_covar", [1e-7, 0.0])
def test_float64_mstep_diag_lies_inside_the_bounds(Dj, M, scale, min_covar):
    import voiceconversion_jl_amd as vc
    S0, S1, S2 = dr.mstep_diag_case(1000 + Dj + M, Dj, M, scale)
    ref = dr.mstep_diag(S0, S1, S2, min_covar)
    bounds = dr.mstep_diag_bounds(S0, S1, S2, min_covar, ref)
    got = vc.mstep_diag(S0, S1, S2, min_covar)
    for name, g, r, b in zip(("w", "mu", "var"), got, ref, bounds):
        assert g.shape == r.shape == b.shape
        excess = np.max(np.abs(np.asarray(g, dtype=LD) - r) / b)
        print(f"({Dj},{M},{scale:g}) min_covar {min_covar:g}: {name} uses {float(excess):.3f} of its bound")
        assert excess <= 1, (name, float(excess))
    # the bounds are not vacuous: they stay far below the quantities themselves where nothing cancels
    assert np.all(bounds[0] <= 1e-14 * np.abs(ref[0])) and np.all(bounds[1] <= 1e-15 * np.abs(ref[1]) + 1e-300)


def test_restatement_follows_the_guards_of_the_old_sklearn_update():
    """An empty mixture: w = eps, mu = 0, var = min_covar -- exactly, in longdouble as in float64."""
    S0 = np.array([3.0, 0.0])
    S1 = np.array([[6.0, 0.0]])
    S2 = np.array([[15.0, 0.0]])
    w, mu, var = dr.mstep_diag(S0, S1, S2, 1e-3)
    assert float(w[1]) == np.finfo(np.float64).eps and float(mu[0, 1]) == 0.0 and var[0, 1] == LD(1e-3)
    assert abs(float(mu[0, 0]) - 2.0) < 1e-14 and abs(float(var[0, 0]) - (1.0 + 1e-3)) < 1e-13


def test_pack_diag_stats_is_the_layout_unpack_stats_reads():
    import voiceconversion_jl_amd as vc
    S0, S1, S2 = dr.mstep_diag_case(5, 3, 4, 1.0)
    p = dr.pack_diag_stats(S0, S1, S2, -7.5)
    assert p.shape == (4 * (1 + 2 * 3) + 1,)
    u0, u1, u2, ll = vc.unpack_stats(p, 3, 4)
    assert np.array_equal(u0, S0) and np.array_equal(u1, S1) and np.array_equal(u2, S2) and ll == -7.5


def test_expand_diag():
    import voiceconversion_jl_amd as vc
    v = np.arange(1.0, 13.0).reshape(3, 4)
    s = vc.expand_diag(v)
    assert s.shape == (3, 3, 4) and s.flags.f_contiguous and s.dtype == np.float64
    for m in range(4):
        assert np.array_equal(s[:, :, m], np.diag(v[:, m]))
    assert vc.expand_diag(np.ones((1, 1))).shape == (1, 1, 1)
    with pytest.raises(vc.DimensionMismatch):
        vc.expand_diag(np.ones(3))
    with pytest.raises(vc.DimensionMismatch):
        vc.expand_diag(np.ones((2, 2, 2)))


def test_train_gmm_argument_errors_come_before_any_device_call():
    """On a machine without a GPU a device call would fail with another exception type: X never leaves the host."""
    import voiceconversion_jl_amd as vc
    X = np.zeros((4, 10))
    with pytest.raises(ValueError, match="covariance_type"):
        vc.train_gmm(X, n_components=2, covariance_type="tied")
    with pytest.raises(ValueError, match="covariance_type"):
        vc.train_gmm(X, n_components=2, covariance_type=None)
    full = (np.full(2, 0.5), np.zeros((4, 2)), np.repeat(np.eye(4)[:, :, None], 2, axis=2))
    with pytest.raises(vc.DimensionMismatch, match="diag"):
        vc.train_gmm(X, n_components=2, covariance_type="diag", refine=full)


def test_recovery_input_converges_and_meets_its_bound_with_a_numpy_em():
    """The input of test_gpu_em_diag.py's recovery test, once through a float64 EM built from the oracle's E-step and
    estep.py:mstep_diag, started from the host k-means++ seeding of train.py: it converges, and every mean lies within 6
    standard errors of the sample mean of its own frames (the mixtures do not overlap, so a correct fit deviates by far less)."""
    import voiceconversion_jl_amd as vc
    from oracle import np_oracle as npo
    from voiceconversion_jl_amd.train import kmeans_init
    X, lab, mu_true, sd = dr.recovery_case()
    N, Dj = X.shape
    M = len(mu_true)
    rng = np.random.default_rng(0)
    mu = kmeans_init(X, M, rng)                                            # (M,Dj)
    var = np.repeat((np.var(X, axis=0, ddof=1) + 1e-7)[None, :], M, axis=0)
    w = np.full(M, 1.0 / M)
    hist = []
    for _ in range(50):
        S0, S1, S2, ll = npo.estep_diag(X, w, mu, var)
        hist.append(ll / N)
        if len(hist) > 1 and abs(hist[-1] - hist[-2]) < 1e-3:
            break
        w, muT, varT = vc.mstep_diag(S0, S1.T, S2.T, 1e-7)
        mu, var = muT.T, varT.T
    assert len(hist) < 50
    worst = dr.recovery_worst_deviation(X, lab, mu_true, mu.T)
    print(f"numpy EM: {len(hist)} iterations, worst mean deviation {worst:.3f} standard errors")
    assert worst <= 6.0
