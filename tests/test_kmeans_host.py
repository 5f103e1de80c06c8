"""CPU: the numpy restatement of k-means that tests/test_gpu_kmeans.py checks the device against, checked in turn against
the installed scikit-learn; and the host-side surface of the feature (exports, statistics layout, train_gmm's init)."""
import inspect

import numpy as np
import pytest

import kmeans_restatement as kr


def separated(seed, M, Dj, n_per, spread=0.05, scale=10.0):
    rng = np.random.default_rng(seed)
    mu = scale * rng.standard_normal((M, Dj))
    comp = np.repeat(np.arange(M), n_per)
    rng.shuffle(comp)
    return mu[comp] + spread * rng.standard_normal((len(comp), Dj)), comp, mu


def test_restatement_matches_sklearn_lloyd_fixed_point():
    sk = pytest.importorskip("sklearn.cluster")
    X, comp, mu = separated(1, 6, 5, 200, spread=0.8, scale=3.0)
    rng = np.random.default_rng(2)
    C0 = X[rng.choice(len(X), 6, replace=False)]
    C, inertia, n_iter, lab, _ = kr.lloyd(X, C0, max_iter=300, tol_abs=0.0)
    ref = sk.KMeans(n_clusters=6, init=C0, n_init=1, algorithm="lloyd", tol=0.0, max_iter=300).fit(X)
    assert np.array_equal(lab, ref.labels_)
    assert np.max(np.abs(C - ref.cluster_centers_)) <= 1e-10 * np.max(np.abs(ref.cluster_centers_))
    assert abs(inertia - ref.inertia_) <= 1e-10 * ref.inertia_


def test_restatement_distances_and_ties():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((50, 7))
    C = rng.standard_normal((4, 7))
    D = kr.direct(X, C)
    assert np.allclose(D, ((X[:, None, :] - C[None]) ** 2).sum(-1), rtol=1e-14, atol=0)
    C2 = np.vstack([C, C[1]])                      # a duplicate of center 1 at index 4: every tie goes to 1
    lab, _ = kr.assign(X, C2)
    assert not np.any(lab == 4)


def test_restatement_relocates_empty_clusters_to_the_farthest_frames():
    X = np.array([[0.0], [0.1], [0.2], [5.0], [5.1], [9.0], [9.0]])
    C0 = np.array([[0.1], [5.05], [100.0], [200.0]])   # clusters 2 and 3 are empty at the first assignment
    lab, d2 = kr.assign(X, C0)
    newC, empty = kr.update(X, C0, lab, d2)
    assert list(empty) == [2, 3]
    # the two 9.0 frames tie on the largest distance: the smaller index (5) goes to the first empty cluster
    assert newC[2, 0] == 9.0 and newC[3, 0] == 9.0
    order = np.lexsort((np.arange(len(X)), -d2))
    assert list(order[:2]) == [5, 6]


def test_restatement_seeding_picks_frames_and_recovers_separated_clusters():
    X, comp, mu = separated(4, 5, 3, 100)
    picks, margin = kr.kpp(X, 5, np.random.default_rng(0))
    assert len(set(picks)) == 5 and margin > 0
    assert len(set(comp[picks])) == 5                 # greedy k-means++ lands one seed in every well-separated cluster
    C, inertia, n_iter, lab = kr.kmeans(X, 5, n_init=2, seed=1)
    for k in range(5):
        assert len(set(lab[comp == k])) == 1


def test_kmeans_is_exported_and_train_gmm_has_an_opt_in_init():
    import sys

    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import _lib

    km = sys.modules["voiceconversion_jl_amd.kmeans"]     # (the package attribute `kmeans` is the function)
    assert callable(vc.kmeans) and vc.kmeans is km.kmeans
    sig = inspect.signature(vc.kmeans)
    assert [p for p in sig.parameters] == ["X", "n_clusters", "n_init", "max_iter", "tol", "seed", "init", "group"]
    assert sig.parameters["n_init"].default == 10 and sig.parameters["max_iter"].default == 300
    assert sig.parameters["tol"].default == 1e-4
    assert inspect.signature(vc.train_gmm).parameters["init"].default == "subsample"
    # [count (M) | sum x (Dj,M) | inertia]
    assert km.kmeans_stats_len(80, 64) == 64 * 81 + 1
    assert _lib.lib.vcmi_kmeans_stats_len(0, 4) == 0
