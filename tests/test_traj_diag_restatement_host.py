"""CPU: the two forms of tests/traj_diag_restatement.py agree -- the reference's sparse-W statement with Dy_m replaced by
diag(q_m), and the per-parity tridiagonal systems the device solves -- to 64 cond 2^-53 on the shapes of the GPU test, cond the
largest condition number of the tridiagonal matrices of that utterance.  What the GPU test compares the device with is
therefore the reference's algorithm under another precision matrix, not a second invention."""
import numpy as np
import pytest

import traj_diag_restatement as R
from conftest import relerr


@pytest.mark.parametrize("D,M,Ts", R.SHAPES)
def test_sparse_and_tridiagonal_forms_agree(D, M, Ts):
    model, Xs = R.make_case(D, M, Ts)
    dt = R.DiagTrajectory(*model)
    assert dt.q.shape == (M, 2 * D) and np.all(dt.q > 0)
    for X in Xs + [np.zeros((0, 2 * D))]:
        a = dt.sparse(X)
        b, cond = dt.tridiag(X)
        assert a.shape == b.shape == (X.shape[0], D)
        if X.shape[0]:
            print(D, X.shape[0], relerr(a, b), cond)
            assert 1.0 <= cond < 10.0                       # strictly diagonally dominant, p_d / p_s moderate
            assert relerr(a, b) < R.tolerance(cond)


def test_q_is_not_the_diagonal_of_the_full_precision():
    model, _ = R.make_case(12, 4, [1])
    dt = R.DiagTrajectory(*model)
    full = np.stack([np.diag(np.linalg.inv(C)) for C in dt.C])
    assert np.max(np.abs(dt.q * np.stack([np.diag(C) for C in dt.C]) - 1.0)) < 1e-15
    assert np.max(np.abs(full / dt.q - 1.0)) > 0.1


def test_special_models():
    """the two other models of the GPU test: diagonal by construction (the off-diagonal conditional covariance is rounding, full
    and diagonal solutions agree), and delta precisions ~1e8 x the static ones (ill-conditioned, yet inside 1e-6)"""
    from oracle import np_oracle as npo
    D, M, T = 12, 4, 50
    model = R.diagonal_conditional_model(71, D, M)
    dt = R.DiagTrajectory(*model)
    assert max(np.max(np.abs(C - np.diag(np.diag(C)))) for C in dt.C) < 1e-13
    X = R.smooth_frames(np.random.default_rng(3), *model, T, D)
    yfull = npo.TrajectoryGMMMap(npo.GMMMap(*model)).fvconvert(X)[0]
    ydiag, cond = dt.tridiag(X)
    assert relerr(ydiag, yfull) < 1e-11
    assert relerr(dt.sparse(X), ydiag) < R.tolerance(cond)
    model = R.ill_conditioned_model(81, D, M)
    dt = R.DiagTrajectory(*model)
    assert 1e7 < np.median(dt.q[:, D:] / dt.q[:, :D]) < 1e9
    X = R.smooth_frames(np.random.default_rng(4), *model, T, D)
    y, cond = dt.tridiag(X)
    assert 1e3 < cond and R.tolerance(cond) < 1e-6
    assert relerr(dt.sparse(X), y) < R.tolerance(cond)
