"""CPU: tests/traj_bdiag_restatement.py -- trajectory conversion written from the cross-diagonal parameters alone -- agrees with
tests/traj_diag_restatement.py's DiagTrajectory on the EXPANDED model (em_bdiag_restatement.expand), in both of its forms: the
reference's sparse-W statement with Dy_m = diag(q_m), and the per-parity tridiagonal systems; within 64 cond rho 2^-53 (derived
in the helper's docstring).  And the conditions the GPU tests (tests/test_gpu_traj_bdiag.py) rest on, for every input they use:
every q > 0, and no undecided frame -- the top-two log-density gap exceeds 2 max_m B_tm on EVERY frame (cap: zero frames), so the
device's arg-max is the restatement's whatever the rounding."""
import numpy as np
import pytest

import traj_bdiag_restatement as R
import traj_diag_restatement as DR
from conftest import relerr


def check_inputs(bt, Xs):
    """-> (smallest gap, largest bound, most distinct mhat in an utterance) after asserting the GPU tests' conditions"""
    assert bt.q.shape == (bt.D2, bt.M) and np.all(bt.q > 0) and np.all(np.isfinite(bt.q))
    gmin, bmax, distinct = np.inf, 0.0, 0
    for X in Xs:
        gap, bound = bt.undecided(X)
        assert int(np.sum(~(gap > bound))) == 0, (gap.min(), bound.max())
        gmin, bmax = min(gmin, float(gap.min())), max(bmax, float(bound.max()))
        distinct = max(distinct, len(np.unique(bt.mhat(X))))
    return gmin, bmax, distinct


@pytest.mark.parametrize("D,M,Ts", R.SHAPES)
def test_against_the_expanded_model(D, M, Ts):
    model, Xs = R.make_case(D, M, Ts)
    bt = R.BdiagTrajectory(*model)
    gmin, bmax, distinct = check_inputs(bt, Xs)
    print(f"D={D} M={M}: smallest gap {gmin:.3g}, largest bound {bmax:.3g}, up to {distinct} distinct mhat")
    assert bmax <= 7.5e-12 and gmin >= 9.6e-4 * 0.999
    dt = DR.DiagTrajectory(*R.expanded_model(*model))
    assert relerr(dt.q.T, bt.q) < 1e-13
    for X in Xs + [np.zeros((0, 2 * D))]:
        y, cond, rho = bt.tridiag(X)
        assert y.shape == (X.shape[0], D)
        if X.shape[0] == 0:
            continue
        assert np.array_equal(bt.mhat(X), dt.g.predict(X))
        yt, cond_t = dt.tridiag(X)
        ys = dt.sparse(X)
        tol = DR.tolerance(cond) * rho
        print(f"  T={X.shape[0]}: tridiag {relerr(y, yt):.3g} sparse {relerr(y, ys):.3g} cond {cond:.3g} rho {rho:.3g} bound {tol:.3g}")
        assert 1.0 <= cond <= 24.3 * 1.001 and rho >= 1.0 and abs(cond - cond_t) <= 1e-9 * cond
        assert relerr(y, yt) < tol and relerr(y, ys) < tol


def test_swap_and_vc_inputs():
    """the swapped case of the GPU test, against the expanded model with its halves exchanged; vc in chunks is tridiag per chunk"""
    D, M, Ts = 12, 4, [1, 2, 3, 4, 5, 50]
    model, Xs = R.make_case(D, M, Ts, swap=True)
    bt = R.BdiagTrajectory(*model, swap=True)
    check_inputs(bt, Xs)
    w, mu, sig = R.expanded_model(*model)
    perm = np.r_[2 * D:4 * D, 0:2 * D]
    dt = DR.DiagTrajectory(w, mu[:, perm], sig[:, perm][:, :, perm])
    for X in Xs:
        y, cond, rho = bt.tridiag(X)
        assert relerr(y, dt.tridiag(X)[0]) < DR.tolerance(cond) * rho
    # the utterance of the vc tests (its first 37 frames are the batch's third utterance; the arg-max is per frame, so chunks
    # and prefixes are decided with it)
    D, M, Ts = R.VC_CASE
    model, (X,) = R.make_case(D, M, Ts)
    bt = R.BdiagTrajectory(*model)
    check_inputs(bt, [X])
    fm = np.concatenate([np.arange(100.0)[:, None], X], axis=1)
    out, cond, rho = bt.vc(fm, 30)
    assert np.array_equal(out[:, 0], fm[:, 0]) and np.array_equal(out[90:, 1:], bt.tridiag(X[90:])[0])
    assert cond >= 1.0 and rho >= 1.0


def test_first_maximum_case_is_decided_between_its_groups():
    """the tie of the GPU test: mixtures 1 and 2 share weight and source side bit for bit (their log-densities are the same
    number on any evaluation that treats mixtures alike), mixture 3 has weight 0 (-inf): the first maximum is mixture 1"""
    model, X = R.tie_case()
    bt = R.BdiagTrajectory(*model)
    from em_bdiag_restatement import pairs_valid
    assert np.all(bt.q > 0) and np.all(pairs_valid(model[2]))
    L = R.BR.logdens(X, *model)
    assert np.array_equal(L[:, 0], L[:, 1]) and np.all(np.isneginf(L[:, 2]))
    assert np.all(bt.mhat(X) == 1)
    assert relerr(bt.tridiag(X)[0], bt.tridiag(X, mhat=np.full(len(X), 2))[0]) > 1e-3      # the target sides differ visibly
