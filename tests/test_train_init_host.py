"""CPU: train_gmm's host-side subsample initialisation (train.py:subsample_model) against the literal expressions of the three
covariance types -- the same arrays, the same draws from the generator -- and the pack / unpack of the rank-0 model that every
rank receives.  tests/test_gpu_train_init.py runs the same expressions through a hand loop on the device."""
import numpy as np
import pytest

KINDS = ("full", "diag", "block_diag")


def literal_subsample_model(kind, Xs, M, rng, min_covar):
    """The initial model of one covariance type from the host subsample Xs (n,Dj), spelled out: uniform weights, the k-means
    means, and for every mixture the covariance entry of the subsample (min_covar on variances only)."""
    from voiceconversion_jl_amd.train import kmeans_init
    Dj = Xs.shape[1]
    mu0 = kmeans_init(Xs, M, rng).T
    if kind == "full":
        third = np.repeat((np.cov(Xs.T) + min_covar * np.eye(Dj))[:, :, None], M, axis=2)
    elif kind == "diag":
        third = np.repeat((np.var(Xs, axis=0, ddof=1) + min_covar)[:, None], M, axis=1)
    else:
        D = Dj // 2
        Xc = Xs - Xs.mean(axis=0)
        pair = (Xc[:, :D] * Xc[:, D:]).sum(axis=0) / (len(Xs) - 1.0)
        floor = np.concatenate([np.full(Dj, float(min_covar)), np.zeros(D)])
        third = np.repeat((np.concatenate([np.var(Xs, axis=0, ddof=1), pair]) + floor)[:, None], M, axis=1)
    return np.full(M, 1.0 / M), mu0, third


def _subsample():
    rng = np.random.default_rng(17)
    A = rng.standard_normal((6, 6))
    return 5.0 * rng.integers(0, 3, 200)[:, None] + rng.standard_normal((200, 6)) @ A       # correlated, three clumps


@pytest.mark.parametrize("kind", KINDS)
def test_subsample_model_is_the_literal_expression_and_draws_the_same(kind):
    from voiceconversion_jl_amd.train import subsample_model
    Xs, M, min_covar = _subsample(), 3, 1e-3
    ra, rb = np.random.default_rng(23), np.random.default_rng(23)
    got = subsample_model(Xs, M, ra, min_covar, kind)
    want = literal_subsample_model(kind, Xs, M, rb, min_covar)
    shape = {"full": (6, 6, M), "diag": (6, M), "block_diag": (9, M)}[kind]
    assert got[0].shape == (M,) and got[1].shape == (6, M) and got[2].shape == shape
    for g, w in zip(got, want):
        assert g.dtype == np.float64 and np.array_equal(g, w)
    assert np.all(got[0] == 1.0 / M)
    assert ra.random() == rb.random()                               # the generator is left where the literal draws leave it
    if kind != "full":                                              # min_covar on variances only
        assert np.array_equal(got[2][:6, 0], np.var(Xs, axis=0, ddof=1) + min_covar)
    if kind == "block_diag":
        cv = np.cov(Xs.T)
        assert np.max(np.abs(got[2][6:, 1] - cv[np.arange(3), np.arange(3) + 3])) <= 1e-12 * np.max(np.abs(cv))


@pytest.mark.parametrize("kind", KINDS)
def test_the_init_error_comes_before_any_collective_or_device_call(kind):
    """X is a host array: anything past the argument checks would fail with another exception type."""
    import voiceconversion_jl_amd as vc
    with pytest.raises(ValueError, match="init must be 'subsample' or 'kmeans', got 'random'"):
        vc.train_gmm(np.zeros((4, 10)), n_components=2, init="random", covariance_type=kind)


@pytest.mark.parametrize("third_shape", [(4, 4, 3), (4, 3), (6, 3)])
def test_pack_and_unpack_of_the_model_are_inverse(third_shape):
    """Non-symmetric content: a transposed (Dj,Dj,M) or (Dj + D, M) would show."""
    from voiceconversion_jl_amd.train import pack_model, unpack_model
    Dj, M = 4, 3
    rng = np.random.default_rng(3)
    w, mu, third = rng.random(M), rng.standard_normal((Dj, M)), rng.standard_normal(third_shape)
    for t in (third, np.asfortranarray(third)):
        p = pack_model(w, mu, t)
        assert p.shape == (M * (1 + Dj) + third.size,) and p.dtype == np.float64
        w2, mu2, t2 = unpack_model(p, Dj, M, third_shape)
        assert w2.shape == (M,) and mu2.shape == (Dj, M) and t2.shape == third_shape
        assert np.array_equal(w2, w) and np.array_equal(mu2, mu) and np.array_equal(t2, third)
