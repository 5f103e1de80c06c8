"""CPU: the long-double reference of tests/traj_full_restatement.py is what it claims to be, and the bar of the GPU test
(tests/test_gpu_traj_full.py: 64 cond 2^-53) is tied to something independent of the device -- oracle/np_oracle.py's
TrajectoryGMMMap (FP64, explicit sparse W, sparse LU) stays within 8 cond 2^-53 of the reference, an eighth of the bar: the
device gets a factor 8 over plain FP64 for its different operation order.  Measured (worst err / (cond 2^-53) of numpy over
D in {12, 13, 16, 20, 24, 25, 30, 32, 35, 40, 41, 46, 47, 64, 65, 72}, the lengths and sequences of the GPU test): 4.4;
on the ill-conditioned variant at D = 12 0.04 (profiles/traj_full_parity/README.md)."""
import numpy as np
import pytest

import traj_full_restatement as R
from conftest import relerr
from oracle import np_oracle as npo

HOST_TS = (1, 2, 3, 5, 13, 33)


def _check_case(D, M, kind, Ts, ill=False):
    mdl, ft, Xs, ss, refs = R.case(D, M, kind, tuple(Ts), ill)
    tj = npo.TrajectoryGMMMap(npo.GMMMap(*mdl))
    worst = 0.0
    for X, s, (y, gap, cond, mh) in zip(Xs, ss, refs):
        T = X.shape[0]
        # the prescribed sequence is the arg-max, beyond dispute
        assert np.array_equal(mh, s) and gap >= R.MIN_GAP, (D, T, gap)
        # the reference solves its own system: long-double residual
        P, r, _, _ = ft.system(X)
        res = float(np.max(np.abs(r - P.matvec(y))) / (P.norm_inf() * np.max(np.abs(y)) + np.max(np.abs(r))))
        assert res < 2.0 ** -58, (D, T, res)
        # the cheap bound is one
        c2, upper = ft.cond(P)
        assert c2 is not None and cond == c2 and upper >= c2, (D, T, c2, upper)
        # plain FP64 by another algorithm
        y64, mh64, _ = tj.fvconvert(X)
        assert np.array_equal(mh64, s)
        err = relerr(y64, y)
        worst = max(worst, err / (cond * R.EPS))
        print(f"D={D} T={T} ill={ill} gap {gap:.1f} cond {cond:.4g} (bound {upper:.4g}) residual {res:.2e} numpy err {err:.3e} "
              f"ratio {err / (cond * R.EPS):.2f}")
        assert err < 8.0 * cond * R.EPS, (D, T, err, cond)
    return worst


@pytest.mark.parametrize("D", [12, 25, 40, 47])
def test_reference_and_numpy_agree(D):
    M, kind = R.SHORT[D]
    _check_case(D, M, kind, HOST_TS)


def test_ill_conditioned_variant():
    """delta rows and columns scaled by 1e-2: cond_2(P) in the thousands, and numpy stays as far inside its bar"""
    mdl, ft, Xs, _, refs = R.case(12, 4, "rand", (50,), True)
    assert refs[0][2] > 1e3 and R.tolerance(refs[0][2]) < 1e-9
    assert _check_case(12, 4, "rand", (50,), ill=True) < 1.0


def test_sequences_and_the_empty_utterance():
    rng = np.random.default_rng(0)
    assert np.array_equal(R.sequence("last", 5, 4, rng), [4, 4, 4, 4])
    assert np.array_equal(R.sequence("cycle", 3, 7, rng), [0, 1, 2, 0, 1, 2, 0])
    s = R.sequence("runs", 32, 150, rng)
    runs = np.diff(np.flatnonzero(np.concatenate([[1], np.diff(s), [1]])))
    assert list(runs) == [15, 16, 17, 1, 31, 32, 33, 5] and list(s[np.cumsum(runs) - 1]) == [0, 3, 6, 9, 12, 15, 18, 21]
    assert len(set(R.sequence("rand", 32, 257, rng))) > 16
    mdl = R.model(R.MODEL_SEED + 12, 12, 4)
    y, gap, cond = R.reference(*mdl, np.zeros((0, 24)))
    assert y.shape == (0, 12) and cond == 1.0
    # above D T = 4000 the condition number is the upper bound
    ft = R.FullTrajectory(*mdl)
    X, _ = R.utterance(mdl, 12, 4, "rand", 340, 1)
    P = ft.system(X)[0]
    c2, upper = ft.cond(P)
    assert c2 is None and ft.reference(X)[2] == upper
    lam = np.linalg.eigvalsh(P.dense64())
    assert lam[-1] / lam[0] <= upper
