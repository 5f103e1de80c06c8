"""GPU: the cross-diagonal ("block_diag") joint GMM on the device -- vcmi_estep_bdiag_dev, vcmi_gmm_em_bdiag_*,
BlockDiagEMState, train_gmm(covariance_type="block_diag").  The E-step against two independent references (the C oracle's and
the device's full-covariance E-step on the expanded model), on a case where an expanded form would cancel, and against the
diagonal E-step; em_mstep_bdiag_kernel against the longdouble restatement and its bounds (tests/em_bdiag_restatement.py, proved
by tests/test_em_bdiag_host.py); the E-step from device parameters bit for bit; the not-positive-definite report; train_gmm
against a hand loop, against sample moments, on two ranks; and the fitted model through TrajectoryGMMMap in both precisions."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr
from test_gpu_estep_adversarial import per_mixture_err

pytestmark = pytest.mark.gpu
TOL = 1e-9
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


@pytest.fixture(scope="module")
def br():
    try:
        import em_bdiag_restatement
    except AssertionError as e:                       # long double is a double here: no silent float64 reference
        pytest.skip(str(e))
    return em_bdiag_restatement


def dev(X):
    """(N,Dj) host frames -> the (Dj,N) device view the library takes"""
    import torch
    return torch.from_numpy(np.array(X, order="C")).cuda().t()       # (a copy: the shared cases are read-only)


def _f64(t):
    return tuple(np.asarray(a, dtype=np.float64) for a in t)


# (Dj, M, N) -- em_bdiag_restatement.ESTEP_BDIAG_SHAPES / ESTEP_BDIAG_NS, spelled out because that module needs an extended long double
ESTEP_SHAPES = [(2, 1, 1), (2, 3, 100), (6, 5, 1000), (34, 17, 3000), (80, 32, 20000), (160, 16, 4096), (256, 2, 500), (8, 256, 2000)]
ESTEP_NS = [63, 64, 65, 4097]


# ------------------------------------------------------------------------------- 1. the E-step against two references
@pytest.mark.parametrize("Dj,M,N", ESTEP_SHAPES + [(16, 4, n) for n in ESTEP_NS])
def test_estep_against_the_oracle_and_the_full_covariance_kernels(vc, br, Dj, M, N):
    """Pair correlations in (-0.9, 0.9), mixtures a few standard deviations apart (they share frames).  The references: the C
    oracle's estep_full on the expanded model, and estep_full_dev on the device on the same frames; their (d,d) and (d,d+D)
    entries against S2 and Sxy.  1e-9 per mixture, loglik 1e-9 relative."""
    assert ESTEP_SHAPES == br.ESTEP_BDIAG_SHAPES and ESTEP_NS == br.ESTEP_BDIAG_NS
    w, mu, cov, Xh = br.estep_case(Dj, M, N)
    X = dev(Xh)
    st = vc.estep_bdiag_dev(X, w, mu, cov)
    assert st.shape == (vc.bdiag_stats_len(Dj, M),) == (M * (1 + 2 * Dj + Dj // 2) + 1,)
    got = vc.unpack_bdiag_stats(st.cpu().numpy(), Dj, M)
    assert got[3].shape == (Dj // 2, M)
    full = vc.unpack_full_stats(vc.estep_full_dev(X, w, mu, vc.expand_block_diag(cov)).cpu().numpy(), Dj, M)
    for name, ref in (("C oracle", br.estep_oracle(Dj, M, N)), ("estep_full_dev", br.full_to_bdiag(*full))):
        e = per_mixture_err(got[:4], ref[:4])
        ell = abs(got[4] - ref[4]) / abs(ref[4])
        print(f"  ({Dj},{M},{N}) against {name}: per-mixture error {e.max():.2e}, loglik {ell:.2e}")
        assert e.max() <= TOL, (name, e)
        assert ell <= TOL, (name, got[4], ref[4])
    # identical inputs give identical bits, whatever ran before
    import torch
    assert torch.equal(st, vc.estep_bdiag_dev(X, w, mu, cov))


# --------------------------------------------------------------------------------------------------- 2. cancellation
def test_estep_where_an_expanded_form_cancels(vc, br):
    """Two mixtures identical except for their weights (gamma is the ratio of the weights), variances 1e-6, |mu| ~ 10, pair
    correlations +-(1 - 1e-6): against the longdouble restatement at 1e-9.  (The kernel evaluates the centred, factorised form
    throughout; the library has no expanded GEMM form of this log-density, so there is no unrepaired figure to quote.  The
    host file checks the C oracle on the same case.)"""
    w, mu, cov, Xh = br.cancellation_case()
    N, Dj = Xh.shape
    ref = _f64(br.estep_bdiag(Xh, w, mu, cov, dtype=br.LD))
    got = vc.unpack_bdiag_stats(vc.estep_bdiag_dev(dev(Xh), w, mu, cov).cpu().numpy(), Dj, 2)
    e = per_mixture_err(got[:4], ref[:4])
    ell = abs(got[4] - ref[4]) / abs(ref[4])
    print(f"  cancellation case: per-mixture error {e.max():.2e}, loglik {ell:.2e}, S0 / N = {got[0] / N}")
    assert e.max() <= TOL and ell <= TOL
    assert np.max(np.abs(got[0] / N - w)) <= TOL


# ------------------------------------------------------------------------------------------ 3. zero cross-covariances
def test_zero_cross_covariances_give_the_diagonal_estep(vc, br):
    Dj, M, N = 16, 4, 5000
    w, mu, cov, Xh = br.estep_case(Dj, M, N)
    cov0 = cov.copy()
    cov0[Dj:] = 0.0
    X = dev(Xh)
    got = vc.unpack_bdiag_stats(vc.estep_bdiag_dev(X, w, mu, cov0).cpu().numpy(), Dj, M)
    d = vc.unpack_stats(vc.estep_diag_dev(X, w, mu, np.asfortranarray(cov0[:Dj])).cpu().numpy(), Dj, M)
    e = per_mixture_err(got[:3], d[:3])
    print(f"  against estep_diag_dev: {e.max():.2e}, loglik {abs(got[4] - d[3]) / abs(d[3]):.2e}")
    assert e.max() <= TOL and abs(got[4] - d[3]) <= TOL * abs(d[3])
    ref = br.estep_bdiag(Xh, w, mu, cov0)
    exy = per_mixture_err((got[0], got[3]), (ref[0], ref[3]))
    print(f"  Sxy against numpy: {exy.max():.2e}")
    assert exy.max() <= TOL


# ------------------------------------------------------------------------------------------------ 4. the M-step kernel
def _fresh_state(vc, Dj, M, min_covar):
    return vc.BlockDiagEMState(np.full(M, 1.0 / M), np.zeros((Dj, M)), np.vstack([np.ones((Dj, M)), np.zeros((Dj // 2, M))]),
                               min_covar=min_covar)


def _check_mstep(br, got, stats4, min_covar):
    ref = br.mstep_bdiag(*stats4, min_covar)
    for name, g, r, b in zip(("w", "mu", "covars"), got, ref, br.mstep_bdiag_bounds(*stats4, min_covar, ref)):
        err = np.abs(g.astype(br.LD) - r)
        print(f"  {name}: {float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0))):.2f} of the bound")
        assert np.all(err <= b), (name, float(np.max(err / np.where(b > 0, b, 1))))


# (Dj, M, mean scale) -- em_bdiag_restatement.MSTEP_BDIAG_SHAPES
MSTEP_SHAPES = [(2, 1, 1.0), (4, 3, 1.0), (26, 5, 1e3), (80, 16, 1.0), (80, 128, 1.0), (160, 3, 1.0), (256, 2, 1e3), (12, 256, 1.0)]


@pytest.mark.parametrize("min_covar", [1e-7, 0.0])
@pytest.mark.parametrize("Dj,M,scale", MSTEP_SHAPES)
def test_mstep_kernel_lies_inside_the_bounds_and_repeats_its_bits(vc, br, Dj, M, scale, min_covar):
    import torch
    assert MSTEP_SHAPES == br.MSTEP_BDIAG_SHAPES
    s4 = br.mstep_bdiag_case(2000 + Dj + M, Dj, M, scale)
    ref = br.mstep_bdiag(*s4, min_covar)
    b = br.mstep_bdiag_bounds(*s4, min_covar, ref)
    # (min_covar = 0 is tested where the case stays positive definite by more than the bound: every one of these does)
    assert np.all(br.pairs_valid(np.vstack([ref[2][:Dj] - b[2][:Dj], np.abs(ref[2][Dj:]) + b[2][Dj:]])))
    stats = torch.from_numpy(br.pack_bdiag_stats(*s4, -123.25)).cuda()
    em = _fresh_state(vc, Dj, M, min_covar)
    assert em.mstep(stats) == -123.25
    got = em.get()
    assert got[0].shape == (M,) and got[1].shape == (Dj, M) and got[2].shape == (Dj + Dj // 2, M)
    _check_mstep(br, got, s4, min_covar)
    # the same statistics, on the same state again and on another one: the same bits
    assert em.mstep(stats) == -123.25
    em2 = _fresh_state(vc, Dj, M, min_covar)
    em2.mstep(stats)
    for a, b2, c in zip(got, em.get(), em2.get()):
        assert np.array_equal(a, b2) and np.array_equal(a, c)


def test_mstep_kernel_empty_mixture_among_256(vc, br):
    import torch
    Dj, M, k = 12, 256, 255
    S0, S1, S2, Sxy = br.mstep_bdiag_case(7, Dj, M, 1.0)
    S0[k], S1[:, k], S2[:, k], Sxy[:, k] = 0.0, 0.0, 0.0, 0.0
    for min_covar in (1e-7, 1e-3):
        em = _fresh_state(vc, Dj, M, min_covar)
        em.mstep(torch.from_numpy(br.pack_bdiag_stats(S0, S1, S2, Sxy, 0.0)).cuda())
        w, mu, cov = em.get()
        assert w[k] == EPS and np.all(mu[:, k] == 0.0) and np.all(cov[:Dj, k] == min_covar) and np.all(cov[Dj:, k] == 0.0)
        _check_mstep(br, (w, mu, cov), (S0, S1, S2, Sxy), min_covar)


# -------------------------------------------------------------------------------- 5. the E-step from device parameters
@pytest.mark.parametrize("Dj,M", [(2, 1), (34, 17), (80, 32), (160, 3), (8, 256)])
def test_estep_from_device_parameters_has_the_bits_of_the_host_parameter_entry(vc, br, Dj, M):
    """After an M-step the handle's parameters exist only on the device: state.estep(X) must equal
    estep_bdiag_dev(X, *state.get()) bit for bit -- one frame, a partial workgroup, and 70 000 frames (69 partial rows)."""
    import torch
    w, mu, cov = br.bdiag_model(300 + Dj + M, Dj, M)
    em = vc.BlockDiagEMState(w, mu, cov)
    em.mstep(em.estep(dev(br.draw(1, w, mu, cov, 2000))))
    params = em.get()
    assert all(np.all(np.isfinite(p)) for p in params) and np.all(br.pairs_valid(params[2]))
    assert not np.array_equal(params[1], mu)                       # the M-step has replaced the initial parameters
    X = dev(br.draw(2, w, mu, cov, 70_000))
    for N in (1, 100, 70_000):
        a = em.estep(X[:, :N])
        b = vc.estep_bdiag_dev(X[:, :N], *params)
        assert a.shape == b.shape == (vc.bdiag_stats_len(Dj, M),)
        assert torch.equal(a, b), (N, float((a - b).abs().max()))
        assert bool(torch.isfinite(a).all())
    # no frames: zeroed statistics, through both entries
    for z in (em.estep(X[:, :0], out=torch.full((vc.bdiag_stats_len(Dj, M),), 7.0, dtype=torch.float64, device="cuda")),
              vc.estep_bdiag_dev(X[:, :0], *params, out=torch.full((vc.bdiag_stats_len(Dj, M),), 7.0, dtype=torch.float64, device="cuda"))):
        assert bool((z == 0).all())


def test_estep_past_one_pass_of_the_two_phases(vc, br):
    """140 000 frames: two passes (131 072 + 8 928), the second accumulated onto the first in a fixed order -- against the sum of
    the two halves' own statistics (1e-12: another order of the same sums) and the same bits on a second call."""
    import torch
    Dj, M, N = 6, 5, 140_000
    w, mu, cov = br.bdiag_model(11, Dj, M)
    X = dev(br.draw(12, w, mu, cov, N))
    a = vc.estep_bdiag_dev(X, w, mu, cov)
    parts = vc.estep_bdiag_dev(X[:, :131_072], w, mu, cov) + vc.estep_bdiag_dev(X[:, 131_072:], w, mu, cov)
    assert float(((a - parts).abs() / parts.abs().clamp_min(1.0)).max()) <= 1e-12
    assert torch.equal(a, vc.estep_bdiag_dev(X, w, mu, cov))


# ------------------------------------------------------------------------------------------------ 6. failure protocol
def _bad_pairs():
    return [("vx = 0", 0.0, None, None), ("vx < 0", -1.0, None, None), ("vy NaN", None, float("nan"), None),
            ("c = sqrt(vx vy)", 4.0, 9.0, 6.0), ("c < -sqrt(vx vy)", 4.0, 9.0, -6.5), ("c NaN", None, None, float("nan"))]


def test_create_reports_the_first_invalid_pair(vc, br):
    """Value checks on valid buffers -- nothing here faults."""
    import torch
    Dj, M, d, m = 6, 3, 1, 2
    w, mu, cov = br.bdiag_model(9, Dj, M)
    for what, vx, vy, c in _bad_pairs():
        bad = cov.copy()
        for row, v in ((d, vx), (d + Dj // 2, vy), (Dj + d, c)):
            if v is not None:
                bad[row, m] = v
        with pytest.raises(vc.PosDefException, match=re.escape(f"({d + 1},{m + 1})")):
            vc.BlockDiagEMState(w, mu, bad)
        with pytest.raises(vc.PosDefException, match=re.escape(f"({d + 1},{m + 1})")):
            vc.estep_bdiag_dev(torch.zeros(10, Dj, dtype=torch.float64, device="cuda").t(), w, mu, bad)
    two = cov.copy()
    two[Dj + 2, 1], two[0, 2] = 100.0, -1.0                         # pairs (3,2) and (1,3): (3,2) comes first in memory
    with pytest.raises(vc.PosDefException, match=re.escape("(3,2)")):
        vc.BlockDiagEMState(w, mu, two)
    # shapes and limits
    with pytest.raises(vc.DimensionMismatch):
        vc.BlockDiagEMState(w, mu, cov[:Dj])
    with pytest.raises(vc.DimensionMismatch, match="even"):
        vc.BlockDiagEMState(np.ones(1), np.zeros((3, 1)), np.ones((4, 1)))
    for Dj2, M2 in ((258, 2), (260, 2), (4, 257)):
        with pytest.raises(vc.DimensionMismatch, match="256"):
            vc.BlockDiagEMState(np.full(M2, 1.0 / M2), np.zeros((Dj2, M2)), np.vstack([np.ones((Dj2, M2)), np.zeros((Dj2 // 2, M2))]))
    em = vc.BlockDiagEMState(w, mu, cov)
    with pytest.raises(vc.DimensionMismatch):
        em.estep(torch.zeros(10, 7, dtype=torch.float64, device="cuda").t())            # the wrong dimension
    with pytest.raises(vc.DimensionMismatch):
        em.estep(torch.zeros(10, 8, dtype=torch.float64, device="cuda")[:, :6].t())      # (6,10), but not dense
    assert bool(torch.isfinite(em.estep(torch.zeros(10, 6, dtype=torch.float64, device="cuda").t())).all())


@pytest.mark.parametrize("bad", [3.0, float("nan")])
@pytest.mark.parametrize("Dj,M,d,m", [(4, 2, 1, 1), (80, 32, 39, 17), (12, 256, 0, 255)])
def test_an_mstep_that_breaks_a_pair_is_reported_latched_and_the_parameters_stay(vc, br, Dj, M, d, m, bad):
    """S0 = 1, S1 = 0, S2 = 1 everywhere: unit variances, c = Sxy.  Sxy = 3 in one (d, m): det = 1 - 9 < 0 (a NaN: det NaN)."""
    import torch
    D = Dj // 2
    w, mu, cov = br.bdiag_model(40 + Dj, Dj, M)
    em = vc.BlockDiagEMState(w, mu, cov)
    X = dev(br.draw(4, w, mu, cov, 64))
    good = em.estep(X)
    S0, S1, S2, Sxy = np.ones(M), np.zeros((Dj, M)), np.ones((Dj, M)), np.zeros((D, M))
    Sxy[d, m] = bad
    with pytest.raises(vc.PosDefException, match=re.escape(f"({d + 1},{m + 1})")):
        em.mstep(torch.from_numpy(br.pack_bdiag_stats(S0, S1, S2, Sxy, -1.0)).cuda())
    for a, b in zip(em.get(), (w, mu, cov)):
        assert np.array_equal(a, b)
    with pytest.raises(vc.PosDefException):
        em.estep(X)
    # the report is latched: statistics that are fine no longer move the parameters either
    with pytest.raises(vc.PosDefException, match=re.escape(f"({d + 1},{m + 1})")):
        em.mstep(good)
    for a, b in zip(em.get(), (w, mu, cov)):
        assert np.array_equal(a, b)


def test_several_broken_pairs_name_the_first_in_memory_order(vc, br):
    import torch
    Dj, M = 80, 128
    em = _fresh_state(vc, Dj, M, 1e-7)
    S0, S1, S2, Sxy = np.ones(M), np.zeros((Dj, M)), np.ones((Dj, M)), np.zeros((Dj // 2, M))
    for d, m in ((5, 100), (39, 3), (0, 4), (17, 127)):
        Sxy[d, m] = 3.0
    for _ in range(2):
        with pytest.raises(vc.PosDefException, match=re.escape("(40,4)")):
            em.mstep(torch.from_numpy(br.pack_bdiag_stats(S0, S1, S2, Sxy, 0.0)).cuda())


# ------------------------------------------------------------------------------------------------------ 7. train_gmm
def test_train_gmm_block_diag_with_refine_has_the_bits_of_a_hand_loop(vc, br):
    import torch
    Dj, M, N = 16, 5, 6000
    w, mu, cov = br.bdiag_model(61, Dj, M)
    X = dev(br.draw(5, w, mu, cov, N))
    rng = np.random.default_rng(62)
    start = (np.full(M, 1.0 / M), mu + 0.05 * rng.standard_normal((Dj, M)), np.vstack([1.5 * cov[:Dj], 0.5 * cov[Dj:]]))
    r = vc.train_gmm(X, n_components=M, n_iter=3, tol=0.0, refine=start, covariance_type="block_diag")
    em = vc.BlockDiagEMState(*start, min_covar=1e-7)
    stats = torch.empty(vc.bdiag_stats_len(Dj, M), dtype=torch.float64, device="cuda")
    lls = []
    for _ in range(3):
        em.estep(X, out=stats)
        lls.append(em.mstep(stats))
    hw, hmu, hcov = em.get()
    assert np.array_equal(r["weights"], hw) and np.array_equal(r["means"], hmu) and np.array_equal(r["covars"], hcov)
    assert set(r) == {"weights", "means", "covars", "n_components", "loglik", "converged", "covariance_type"}
    assert r["covars"].shape == (Dj + Dj // 2, M) and r["means"].shape == (Dj, M) and r["weights"].shape == (M,)
    assert r["covariance_type"] == "block_diag" and r["n_components"] == M
    assert r["loglik"] == [v / N for v in lls] and r["converged"] is False
    assert lls[0] < lls[1] < lls[2]                                 # EM ascends
    assert np.any(hcov[Dj:] != 0.0)
    # ... and the expanded model starts the full-covariance fit no lower than the block-diagonal fit ended
    f = vc.train_gmm(X, n_components=M, n_iter=2, tol=0.0, refine=(hw, hmu, vc.expand_block_diag(hcov)))
    print(f"  block_diag loglik {r['loglik']}, full from its expansion {f['loglik']}")
    assert f["covars"].shape == (Dj, Dj, M) and f["loglik"][0] >= r["loglik"][-1] - 1e-9 * abs(r["loglik"][-1])


def test_train_gmm_block_diag_from_the_subsample_initialisation(vc, br):
    """init="subsample": variances and pair covariances of the subsample the means come from; the same call twice gives the same bits"""
    Xh, lab = br.recovery_case()
    a = vc.train_gmm(dev(Xh), n_components=3, n_init=2, n_iter=30, covariance_type="block_diag", seed=3)
    b = vc.train_gmm(dev(Xh), n_components=3, n_init=2, n_iter=30, covariance_type="block_diag", seed=3)
    assert a["covars"].shape == (6, 3) and np.all(br.pairs_valid(a["covars"])) and np.isfinite(a["loglik"]).all()
    assert np.array_equal(a["means"], b["means"]) and np.array_equal(a["covars"], b["covars"]) and a["loglik"] == b["loglik"]


def test_data_block_covariance_is_the_sample_covariance(vc, br):
    from voiceconversion_jl_amd.train import data_block_covariance
    Xh, _ = br.recovery_case()
    got = data_block_covariance(dev(Xh))
    cv = np.cov(Xh.T)
    want = np.concatenate([np.diag(cv), [cv[0, 2], cv[1, 3]]])
    assert got.shape == (6,) and np.max(np.abs(got - want) / np.abs(want)) <= 1e-9


# ------------------------------------------------------------------------- 8. recovery without a statistical threshold
def test_train_gmm_block_diag_recovers_the_sample_moments_of_a_separated_model(vc, br):
    """Three mixtures 20 standard deviations apart, pair correlation 0.8, init="kmeans", n_init=1: every responsibility is 0 or
    1 to far below a rounding (S0 under the fitted model is exactly the integer count of every mixture's own frames), so the
    fitted mu, var - min_covar and c are the ddof = 0 sample moments of those frames, to 1e-9."""
    Xh, lab = br.recovery_case()
    N, Dj = Xh.shape
    r = vc.train_gmm(dev(Xh), n_components=3, n_init=1, init="kmeans", covariance_type="block_diag")
    assert r["converged"] and r["covars"].shape == (6, 3) and r["covariance_type"] == "block_diag"
    S0 = vc.unpack_bdiag_stats(vc.estep_bdiag_dev(dev(Xh), r["weights"], r["means"], r["covars"]).cpu().numpy(), Dj, 3)[0]
    match = [int(np.argmin([np.sum((Xh[lab == m].mean(axis=0) - r["means"][:, k]) ** 2) for m in range(3)])) for k in range(3)]
    assert sorted(match) == [0, 1, 2]
    worst = 0.0
    for k, m in enumerate(match):
        own = Xh[lab == m]
        assert S0[k] == float(len(own))                             # responsibilities exactly 0 or 1
        mean = own.mean(axis=0)
        dvt = own - mean
        var = (dvt * dvt).mean(axis=0)
        c = (dvt[:, :2] * dvt[:, 2:]).mean(axis=0)
        assert abs(c[0] / np.sqrt(var[0] * var[2]) - 0.8) < 0.05
        for got, want in ((r["means"][:, k], mean), (r["covars"][:Dj, k] - 1e-7, var), (r["covars"][Dj:, k], c)):
            worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
        assert abs(r["weights"][k] - len(own) / N) <= 1e-12
    print(f"  {len(r['loglik'])} iterations, worst relative deviation from the sample moments {worst:.2e}")
    assert worst <= TOL


# ---------------------------------------------------------------------------------------------------- 9. two ranks
def _two_rank_case():
    import em_bdiag_restatement as br
    Dj, M, N = 16, 3, 8192
    w, mu, cov = br.bdiag_model(91, Dj, M, sep=3.0)
    start = br.bdiag_model(91, Dj, M, sep=3.3)
    return Dj, M, N, br.draw(8, w, mu, cov, N), start


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import dist as vd

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    Dj, M, N, X, start = _two_rank_case()
    lo, hi = vd.shard_range(N, rank, world)
    r = vc.train_gmm(torch.from_numpy(X[lo:hi]).cuda().t(), n_components=M, n_iter=3, tol=0.0, refine=start, covariance_type="block_diag")
    q.put((rank, {k: r[k] for k in ("weights", "means", "covars", "loglik")}))
    dist.destroy_process_group()


def test_two_rank_train_gmm_block_diag_matches_single_process(vc, br):
    """Two gloo ranks on the one GPU, half of 8192 frames each, one all-reduce of the packed statistics per iteration: the
    parameters match the single-process fit to 1e-12 relative (sums taken in a different order), both ranks hold the same bits."""
    import queue
    import torch
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() % 90)
    procs, res = [], {}
    try:
        for rk in range(2):
            if any(p.exitcode not in (None, 0) for p in procs):    # no rank is started after a failure
                break
            procs.append(ctx.Process(target=_rank_worker, args=(rk, 2, port, q)))
            procs[-1].start()
        assert len(procs) == 2
        for _ in procs:                                            # every child under its own limit
            try:
                rank, out = q.get(timeout=120)
            except queue.Empty:
                pytest.fail(f"a rank did not answer within its limit (exit codes {[p.exitcode for p in procs]})")
            res[rank] = out
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    Dj, M, N, X, start = _two_rank_case()
    ref = vc.train_gmm(torch.from_numpy(X).cuda().t(), n_components=M, n_iter=3, tol=0.0, refine=start, covariance_type="block_diag")
    for rank in (0, 1):
        for k in ("weights", "means", "covars"):
            err = np.max(np.abs(res[rank][k] - ref[k])) / np.max(np.abs(ref[k]))
            print(f"  rank {rank} {k}: {err:.2e}")
            assert err <= 1e-12, (rank, k, err)
        assert np.allclose(res[rank]["loglik"], ref["loglik"], rtol=1e-12, atol=0)
    for k in ("weights", "means", "covars"):
        assert np.array_equal(res[0][k], res[1][k])
    assert res[0]["loglik"] == res[1]["loglik"]


# ----------------------------------------------------------------------------------------- 10. the point of the feature
def test_a_fitted_block_diag_model_converts_exactly_with_diagonal_precisions(vc, br):
    """Fit block_diag on [x; dx; y; dy] features (static D = 4, M = 3, 4000 frames), expand it, and convert an utterance with
    TrajectoryGMMMap in both precisions.  The conditional covariance of a cross-diagonal model IS diagonal: the diagonal mode
    agrees with the tridiagonal restatement within its tolerance(cond), and the full mode with the same reference within the
    bar of test_gpu_traj_diag.py::test_diagonal_by_construction_ties_both_modes_to_the_oracle (1e-6)."""
    import traj_diag_restatement as R
    from test_gpu_traj_diag import TOL_ORACLE
    D, M, N, T = 4, 3, 4000, 60
    Dj = 4 * D
    w0, mu0, cov0 = br.bdiag_model(101, Dj, M, sep=6.0)
    r = vc.train_gmm(dev(br.draw(102, w0, mu0, cov0, N)), n_components=M, n_init=1, init="kmeans", n_iter=30, covariance_type="block_diag")
    assert np.all(br.pairs_valid(r["covars"])) and np.all(np.abs(r["covars"][Dj:]) > 0)
    sigma = vc.expand_block_diag(r["covars"])
    model = (r["weights"], np.ascontiguousarray(r["means"].T), np.ascontiguousarray(np.transpose(sigma, (2, 1, 0))))
    dt = R.DiagTrajectory(*model)
    assert max(np.max(np.abs(C - np.diag(np.diag(C)))) for C in dt.C) < 1e-13
    X = R.smooth_frames(np.random.default_rng(5), *model, T, D)
    ref, cond = dt.tridiag(X)
    t = vc.TrajectoryGMMMap(vc.GMMMap(r["weights"], r["means"], sigma), T)
    yfull = vc.fvconvert(t, X.T)
    t.precision = "diag"
    ydiag = vc.fvconvert(t, X.T)
    ed, ef = relerr(ydiag, ref.T), relerr(yfull, ref.T)
    print(f"  diag vs restatement {ed:.3e} (cond {cond:.3f}, bound {R.tolerance(cond):.3e}), full vs restatement {ef:.3e}")
    assert ydiag.shape == ref.T.shape and ed < R.tolerance(cond)
    assert ef < TOL_ORACLE
