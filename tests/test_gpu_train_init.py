"""GPU: train_gmm from the subsample initialisation has the bits of a hand loop, for the three covariance types -- the draws
from the generator (one rng.choice and one kmeans_init per initialisation, carried from one initialisation to the next), the
covariance entry of the subsample, the Julia shapes handed to the state and the first-strictly-best selection over n_init."""
import numpy as np
import pytest

from test_train_init_host import literal_subsample_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def _frames(kind):
    """600 frames of the separated Dj = 4, M = 3 cases"""
    if kind == "block_diag":
        import em_bdiag_restatement as br
        return br.recovery_case(N=600)[0]
    import em_diag_restatement as dr
    return dr.recovery_case(N=600)[0]


@pytest.mark.parametrize("kind,state", [("full", "EMState"), ("diag", "DiagEMState"), ("block_diag", "BlockDiagEMState")])
def test_train_gmm_from_a_subsample_has_the_bits_of_a_hand_loop(vc, kind, state):
    import torch
    M, n_init, n_iter, seed, sample, min_covar = 3, 3, 4, 5, 200, 1e-7
    Xh = _frames(kind)
    N, Dj = Xh.shape
    assert (N, Dj) == (600, 4)
    X = torch.from_numpy(np.array(Xh, order="C")).cuda().t()
    r = vc.train_gmm(X, n_components=M, n_init=n_init, n_iter=n_iter, tol=0.0, seed=seed, init_sample=sample, covariance_type=kind)

    rng = np.random.default_rng(seed)
    best, finals = None, []
    for _ in range(n_init):
        idx = rng.choice(N, sample, replace=False)
        Xs = np.ascontiguousarray(Xh[np.sort(idx)])
        em = getattr(vc, state)(*literal_subsample_model(kind, Xs, M, rng, min_covar), min_covar=min_covar)
        hist = []
        for _ in range(n_iter):
            hist.append(em.mstep(em.estep(X)) / float(N))
        finals.append(hist[-1])
        if best is None or hist[-1] > best[0]:
            best = (hist[-1], em.get(), hist)
    print(f"  {kind}: final log-likelihoods per frame {finals}")
    w, mu, cov = best[1]
    assert r["covars"].shape == {"full": (Dj, Dj, M), "diag": (Dj, M), "block_diag": (Dj + Dj // 2, M)}[kind]
    assert np.array_equal(r["weights"], w) and np.array_equal(r["means"], mu) and np.array_equal(r["covars"], cov)
    assert r["loglik"] == best[2] and r["converged"] is False and r["n_components"] == M
    assert r.get("covariance_type") == (None if kind == "full" else kind)
