"""CPU: the extended-precision restatement of the full-covariance EM blocks (tests/em_restatement.py) that
tests/test_gpu_em_blocks.py judges the device by, proved first -- against 50-digit mpmath, against the float64 oracles,
and (the M-step error bounds) against plain float64 numpy."""
import numpy as np
import pytest

import em_restatement as er


def _mp_logdens(x, mu, S, digits=50):
    """log N(x; mu, S) with an mpmath Cholesky and forward substitution at `digits` decimal digits."""
    mp = pytest.importorskip("mpmath")
    with mp.workdps(digits):
        n = len(mu)
        A = [[mp.mpf(float(S[min(r, c), max(r, c)])) for c in range(n)] for r in range(n)]      # Hermitian(S)
        L = [[mp.mpf(0)] * n for _ in range(n)]
        for j in range(n):
            d = A[j][j] - mp.fsum(L[j][k] ** 2 for k in range(j))
            assert d > 0
            L[j][j] = mp.sqrt(d)
            for i in range(j + 1, n):
                L[i][j] = (A[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
        b = [mp.mpf(float(x[i])) - mp.mpf(float(mu[i])) for i in range(n)]
        z = []
        for i in range(n):
            z.append((b[i] - mp.fsum(L[i][k] * z[k] for k in range(i))) / L[i][i])
        logdet = 2 * mp.fsum(mp.log(L[i][i]) for i in range(n))
        return -(n * mp.log(2 * mp.pi) + logdet) / 2 - mp.fsum(v * v for v in z) / 2


@pytest.mark.parametrize("cond", [1e2, 1e8, 1e11])
def test_logdens_against_50_digit_mpmath(cond):
    """Dj = 16, 12 drawn frames and the 8 eigen-direction probes.  Largest error relative to |log-density|, measured when
    this test was written: longdouble 1.4e-16 / 4.2e-14 / 4.9e-12 at cond 1e2 / 1e8 / 1e11, float64 LAPACK (the numpy oracle)
    1.4e-13 / 1.5e-11 / 1.9e-8 (one frame of the first rung has a log-density near 0, which inflates both of its figures alike)
    -- the restatement is asserted at least 100 x closer to the truth than float64 at every rung,
    which is what makes it a reference for a float64 kernel."""
    mp = pytest.importorskip("mpmath")
    from oracle import np_oracle as npo
    Dj = 16
    S = er.spd(40 + int(np.log10(cond)), Dj, cond)
    mu = np.random.default_rng(41).standard_normal(Dj)
    drawn, probes = er.probe_frames(42, mu, S, 12)
    X = np.concatenate([drawn, probes])
    w, sig = np.ones(1), S.T[None, :, :].copy()
    ld = er.logdens(X, w, mu[None, :], sig)[:, 0]
    f64 = np.array([npo.estep_full(x[None, :], w, mu[None, :], sig)[3] for x in X])
    e_ld = e_64 = 0.0
    for n, x in enumerate(X):
        t = _mp_logdens(x, mu, S)
        with mp.workdps(50):
            hi = float(ld[n])                              # longdouble -> mpf exactly, as a sum of two doubles
            e_ld = max(e_ld, float(abs(mp.mpf(hi) + mp.mpf(float(ld[n] - er.LD(hi))) - t) / abs(t)))
            e_64 = max(e_64, float(abs(mp.mpf(float(f64[n])) - t) / abs(t)))
    print(f"cond {cond:g}: longdouble {e_ld:.2e}  float64 {e_64:.2e}")
    assert e_ld * 100 <= e_64, (e_ld, e_64)


def test_chol_reads_the_upper_triangle_and_reports_bad_pivots():
    S = er.spd(1, 9, 1e3)
    junk = S.copy()
    junk[np.tril_indices(9, -1)] = np.nan
    assert np.array_equal(er.chol(junk), er.chol(S))
    L = er.chol(S)
    assert np.max(np.abs((L @ L.T).astype(np.float64) - S)) < 1e-17
    with pytest.raises(np.linalg.LinAlgError):
        er.chol(-S)
    Z = np.array([[4.0, 4.0, 1.0], [4.0, 4.0, 1.0], [1.0, 1.0, 9.0]])       # second pivot exactly 0
    with pytest.raises(np.linalg.LinAlgError):
        er.chol(Z)
    bad = S.copy()
    bad[2, 5] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        er.chol(bad)


def test_estep_and_mstep_against_the_float64_oracles():
    from oracle import np_oracle as npo
    from voiceconversion_jl_amd.estep import mstep_full
    Dj, M, N = 12, 3, 400
    w, mu, sig = npo.synth_model(3, Dj, M, lam_lo=1e-1)
    X = npo.sample_frames(4, w, mu, sig, N, 0, Dj)
    got = er.estep_full(X, w, mu, sig)
    ref = npo.estep_full(X, w, mu, sig)
    for g, r in zip(got[:3], ref[:3]):
        assert np.max(np.abs(g.astype(np.float64) - r)) <= 1e-12 * np.max(np.abs(r))
    assert abs(float(got[3]) - ref[3]) <= 1e-12 * abs(ref[3])
    S0, S1, S2 = ref[0], ref[1].T, np.transpose(ref[2], (2, 1, 0))
    for mc in (1e-7, 0.0):
        for g, r in zip(er.mstep_full(S0, S1, S2, mc), mstep_full(S0, S1, S2, mc)):
            assert np.max(np.abs(g.astype(np.float64) - r)) <= 1e-12 * np.max(np.abs(r))


@pytest.mark.parametrize("Dj,M,scale", er.MSTEP_SHAPES)
def test_mstep_bounds_hold_for_float64_numpy(Dj, M, scale):
    """The operation-count bounds the device M-step is held to (em_restatement.mstep_bounds) are attainable: plain float64
    numpy (estep.py:mstep_full) stays inside them on every shape -- at most 0.54 of the bound when this was written."""
    from voiceconversion_jl_amd.estep import mstep_full
    S0, S1, S2 = er.mstep_case(100 + Dj + M, Dj, M, scale)
    worst = 0.0
    for mc in (1e-7, 0.0):
        ref = er.mstep_full(S0, S1, S2, mc)
        got = mstep_full(S0, S1, S2, mc)
        for g, r, b in zip(got, ref, er.mstep_bounds(S0, S1, S2, mc, ref)):
            worst = max(worst, float(np.max(np.abs(g.astype(er.LD) - r) / b)))
    print(f"Dj {Dj} M {M}: float64 numpy at {worst:.2f} of the bound")
    assert worst <= 1.0
