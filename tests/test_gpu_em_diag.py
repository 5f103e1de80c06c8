"""GPU: the device-resident diagonal EM loop (vcmi_gmm_em_diag_*, DiagEMState, train_gmm(covariance_type="diag")) --
em_mstep_diag_kernel against the longdouble restatement and its bounds (tests/em_diag_restatement.py, proved by
tests/test_em_diag_host.py), the E-step from device parameters against the host-parameter entry bit for bit, one whole
iteration against the C oracle, the not-positive report, train_gmm against a hand loop, against the truth and on two ranks,
and the diagonal and full-covariance kernel families against each other."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
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
def dr():
    try:
        import em_diag_restatement
    except AssertionError as e:                       # long double is a double here: no silent float64 reference
        pytest.skip(str(e))
    return em_diag_restatement


def dev(X):
    """(N,Dj) host frames -> the (Dj,N) device view the library takes"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(X)).cuda().t()


def diag_model(seed, Dj, M, spread=4.0, var_lo=0.05):
    """w (M,), mu (Dj,M), var (Dj,M): means spread * N(0,1), variances log-uniform in [var_lo, 1]"""
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(4.0 * np.ones(M))
    mu = np.asfortranarray(spread * rng.standard_normal((Dj, M)))
    var = np.asfortranarray(np.exp(rng.uniform(np.log(var_lo), 0.0, (Dj, M))))
    return w, mu, var


def draw(seed, w, mu, var, N):
    """(N,Dj) frames of the model"""
    rng = np.random.default_rng(seed)
    comp = rng.choice(len(w), size=N, p=w)
    return mu.T[comp] + rng.standard_normal((N, mu.shape[0])) * np.sqrt(var.T[comp])


# ------------------------------------------------------------------------------------------------ 1. the M-step kernel
def _fresh_state(vc, Dj, M, min_covar):
    return vc.DiagEMState(np.full(M, 1.0 / M), np.zeros((Dj, M)), np.ones((Dj, M)), min_covar=min_covar)


def _check_mstep(dr, got, S0, S1, S2, min_covar):
    ref = dr.mstep_diag(S0, S1, S2, min_covar)
    for name, g, r, b in zip(("w", "mu", "var"), got, ref, dr.mstep_diag_bounds(S0, S1, S2, min_covar, ref)):
        err = np.abs(g.astype(dr.LD) - r)
        print(f"  {name}: {float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0))):.2f} of the bound")
        assert np.all(err <= b), (name, float(np.max(err / np.where(b > 0, b, 1))))


# (Dj, M, mean scale) -- em_diag_restatement.MSTEP_DIAG_SHAPES, spelled out because that module needs an extended long double
MSTEP_SHAPES = [(1, 1, 1.0), (2, 3, 1.0), (25, 5, 1e3), (80, 16, 1.0), (80, 128, 1.0), (160, 3, 1.0), (256, 2, 1e3),
                (12, 257, 1.0), (8, 600, 10.0)]


@pytest.mark.parametrize("min_covar", [1e-7, 0.0])
@pytest.mark.parametrize("Dj,M,scale", MSTEP_SHAPES)
def test_mstep_kernel_lies_inside_the_bounds_and_repeats_its_bits(vc, dr, Dj, M, scale, min_covar):
    import torch
    assert MSTEP_SHAPES == dr.MSTEP_DIAG_SHAPES
    S0, S1, S2 = dr.mstep_diag_case(1000 + Dj + M, Dj, M, scale)
    ref = dr.mstep_diag(S0, S1, S2, min_covar)
    # (min_covar = 0 is tested where the case stays positive: every one of these does, by a wide margin)
    assert np.all(ref[2] - dr.mstep_diag_bounds(S0, S1, S2, min_covar, ref)[2] > 0)
    stats = torch.from_numpy(dr.pack_diag_stats(S0, S1, S2, -123.25)).cuda()
    em = _fresh_state(vc, Dj, M, min_covar)
    assert em.mstep(stats) == -123.25
    got = em.get()
    assert got[0].shape == (M,) and got[1].shape == (Dj, M) and got[2].shape == (Dj, M)
    _check_mstep(dr, got, S0, S1, S2, min_covar)
    # the same statistics, on the same state again and on another one: the same bits
    assert em.mstep(stats) == -123.25
    em2 = _fresh_state(vc, Dj, M, min_covar)
    em2.mstep(stats)
    for a, b, c in zip(got, em.get(), em2.get()):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_mstep_kernel_empty_mixture_among_257(vc, dr):
    import torch
    Dj, M, k = 12, 257, 256
    S0, S1, S2 = dr.mstep_diag_case(7, Dj, M, 1.0)
    S0[k], S1[:, k], S2[:, k] = 0.0, 0.0, 0.0
    for min_covar in (1e-7, 1e-3):
        em = _fresh_state(vc, Dj, M, min_covar)
        em.mstep(torch.from_numpy(dr.pack_diag_stats(S0, S1, S2, 0.0)).cuda())
        w, mu, var = em.get()
        assert w[k] == EPS and np.all(mu[:, k] == 0.0) and np.all(var[:, k] == min_covar)
        _check_mstep(dr, (w, mu, var), S0, S1, S2, min_covar)


# -------------------------------------------------------------------------------- 2. the E-step from device parameters
DEVICE_ROUTE = [(2, 1), (32, 16), (80, 32), (82, 17), (80, 128), (160, 3)]
FALLBACK = [(25, 5), (12, 257), (162, 2)]


@pytest.mark.parametrize("Dj,M", DEVICE_ROUTE + FALLBACK)
def test_estep_from_device_parameters_has_the_bits_of_the_host_parameter_entry(vc, Dj, M):
    """After an M-step the handle's parameters exist only on the device.  state.estep(X) must equal estep_diag_dev(X,
    *state.get()) bit for bit: the same values through the same preparation kernels (the device route), or through the
    host-parameter path itself (the fallback shapes).  70 000 frames are past the threshold of the hard-assignment path."""
    import torch
    w, mu, var = diag_model(300 + Dj + M, Dj, M)
    em = vc.DiagEMState(w, mu, var)
    em.mstep(em.estep(dev(draw(1, w, mu, var, 2000))))
    params = em.get()
    assert all(np.all(np.isfinite(p)) for p in params) and np.all(params[2] > 0)
    assert not np.array_equal(params[1], mu)                       # the M-step has replaced the initial parameters
    X = dev(draw(2, w, mu, var, 70_000))
    paths = (vc.ESTEP_AUTO, vc.ESTEP_HARD, vc.ESTEP_SOFT) if (Dj, M) == (80, 32) else (vc.ESTEP_AUTO,)
    try:
        for path in paths:
            vc.estep_set_path(path)
            for N in (1, 100, 70_000):
                a = em.estep(X[:, :N])
                b = vc.estep_diag_dev(X[:, :N], *params)
                assert a.shape == b.shape == (vc.stats_len(Dj, M),)
                assert torch.equal(a, b), (path, N, float((a - b).abs().max()))
                assert bool(torch.isfinite(a).all())
    finally:
        vc.estep_set_path(vc.ESTEP_AUTO)
    # no frames: zeroed statistics
    z = em.estep(X[:, :0], out=torch.full((vc.stats_len(Dj, M),), 7.0, dtype=torch.float64, device="cuda"))
    assert bool((z == 0).all())


# ------------------------------------------------------------------ 3. one iteration against an independent reference
@pytest.mark.parametrize("Dj,M,N", [(8, 4, 4096), (80, 32, 20_000)])
def test_one_iteration_against_the_oracle_and_the_longdouble_mstep(vc, dr, Dj, M, N):
    """Frames of a separated diagonal model with one mixture of variance 1e-6 (the exact re-evaluation of its log-densities
    takes part).  The reference starts from the device's own get(): the C oracle's E-step, then the longdouble M-step --
    against the device's next get(), 1e-9 per mixture (the header's contract for the E-step, carried through the M-step).
    The M-step's S2 / S0 - mu^2 multiplies a relative error of the statistics by mu^2 / var: the tight mixture sits near the
    origin (mu^2 / var of order 1e3), the others have mu^2 / var up to 1e4 -- a float64 sum of the statistics keeps 1e-9 there."""
    from oracle import c_oracle as co
    w, mu, var = diag_model(500 + Dj, Dj, M, spread=3.0, var_lo=0.01)
    var[:, M - 1] = 1e-6
    mu[:, M - 1] = 0.05 * np.random.default_rng(9).standard_normal(Dj)
    Xh = draw(3, w, mu, var, N)
    X = dev(Xh)
    em = vc.DiagEMState(w, mu, var)
    for it in range(2):                                            # from the given and from M-step-made parameters
        p0 = em.get()
        r0, r1, r2, rll = co.estep_diag(Xh, p0[0], np.ascontiguousarray(p0[1].T), np.ascontiguousarray(p0[2].T))
        ref = dr.mstep_diag(r0, r1.T, r2.T, 1e-7)
        ll = em.mstep(em.estep(X))
        got = em.get()
        e = per_mixture_err(got, tuple(np.asarray(r, dtype=np.float64) for r in ref))
        print(f"  ({Dj},{M}) iteration {it}: per-mixture error {e.max():.2e}, loglik {abs(ll - rll) / abs(rll):.2e}")
        assert e.max() <= TOL, e
        assert abs(ll - rll) <= TOL * abs(rll), (ll, rll)


# ------------------------------------------------------------------------------------------------ 4. failure protocol
@pytest.mark.parametrize("bad", [0.5, float("nan")])
@pytest.mark.parametrize("Dj,M,d,m", [(3, 2, 1, 1), (80, 32, 79, 17), (12, 257, 0, 256)])
def test_a_variance_that_is_not_positive_is_reported_and_the_parameters_stay(vc, dr, Dj, M, d, m, bad):
    """S0 = 1, S1 = 1, S2 = 0.5 in one (d, m): mu = 1, var = 0.5 - 2 + 1 + min_covar < 0 (a NaN statistic: var = NaN).
    Value checks on valid buffers -- nothing here faults."""
    import torch
    w, mu, var = diag_model(40 + Dj, Dj, M)
    em = vc.DiagEMState(w, mu, var)
    X = dev(draw(4, w, mu, var, 64))
    good = em.estep(X)
    S0, S1, S2 = np.ones(M), np.zeros((Dj, M)), np.ones((Dj, M))
    S1[d, m], S2[d, m] = 1.0, bad
    with pytest.raises(vc.PosDefException, match=re.escape(f"({d + 1},{m + 1})")):
        em.mstep(torch.from_numpy(dr.pack_diag_stats(S0, S1, S2, -1.0)).cuda())
    for a, b in zip(em.get(), (w, mu, var)):
        assert np.array_equal(a, b)
    with pytest.raises(vc.PosDefException):
        em.estep(X)
    # the report is latched: statistics that are fine no longer move the parameters either
    with pytest.raises(vc.PosDefException, match=re.escape(f"({d + 1},{m + 1})")):
        em.mstep(good)
    for a, b in zip(em.get(), (w, mu, var)):
        assert np.array_equal(a, b)


def test_several_bad_variances_name_the_first_in_memory_order(vc, dr):
    import torch
    Dj, M = 80, 128
    em = _fresh_state(vc, Dj, M, 1e-7)
    S0, S1, S2 = np.ones(M), np.zeros((Dj, M)), np.ones((Dj, M))
    for d, m in ((5, 100), (79, 3), (0, 4), (17, 127)):
        S1[d, m], S2[d, m] = 1.0, 0.5
    for _ in range(2):
        with pytest.raises(vc.PosDefException, match=re.escape("(80,4)")):
            em.mstep(torch.from_numpy(dr.pack_diag_stats(S0, S1, S2, 0.0)).cuda())


def test_create_and_estep_argument_errors(vc):
    import torch
    w, mu, var = diag_model(9, 6, 3)
    for v in (0.0, -1.0, float("nan")):
        bad = var.copy()
        bad[4, 2] = v
        with pytest.raises(vc.PosDefException, match=re.escape("(5,3)")):
            vc.DiagEMState(w, mu, bad)
    with pytest.raises(vc.DimensionMismatch):
        vc.DiagEMState(w, mu, var[:, :2])
    with pytest.raises(vc.DimensionMismatch):
        vc.DiagEMState(np.full(2, 0.5), np.zeros((260, 2)), np.ones((260, 2)))
    em = vc.DiagEMState(w, mu, var)
    with pytest.raises(vc.DimensionMismatch):
        em.estep(torch.zeros(10, 7, dtype=torch.float64, device="cuda").t())            # the wrong dimension
    with pytest.raises(vc.DimensionMismatch):
        em.estep(torch.zeros(10, 8, dtype=torch.float64, device="cuda")[:, :6].t())      # (6,10), but not dense
    assert bool(torch.isfinite(em.estep(torch.zeros(10, 6, dtype=torch.float64, device="cuda").t())).all())


# ------------------------------------------------------------------------------------------------ 5. train_gmm
def test_train_gmm_diag_with_refine_has_the_bits_of_a_hand_loop(vc):
    import torch
    Dj, M, N = 16, 5, 6000
    w, mu, var = diag_model(61, Dj, M)
    X = dev(draw(5, w, mu, var, N))
    rng = np.random.default_rng(62)
    start = (np.full(M, 1.0 / M), mu + 0.3 * rng.standard_normal((Dj, M)), 1.5 * var)
    r = vc.train_gmm(X, n_components=M, n_iter=3, tol=0.0, refine=start, covariance_type="diag")
    em = vc.DiagEMState(*start, min_covar=1e-7)
    stats = torch.empty(vc.stats_len(Dj, M), dtype=torch.float64, device="cuda")
    lls = []
    for _ in range(3):
        em.estep(X, out=stats)
        lls.append(em.mstep(stats))
    hw, hmu, hvar = em.get()
    assert np.array_equal(r["weights"], hw) and np.array_equal(r["means"], hmu) and np.array_equal(r["covars"], hvar)
    assert r["covars"].shape == (Dj, M) and r["covariance_type"] == "diag" and r["n_components"] == M
    assert r["loglik"] == [v / N for v in lls] and r["converged"] is False
    assert lls[0] < lls[2]                                          # EM ascends
    # ... and warm-starts the full-covariance fit
    f = vc.train_gmm(X, n_components=M, n_iter=2, tol=0.0, refine=(hw, hmu, vc.expand_diag(hvar)))
    assert f["covars"].shape == (Dj, Dj, M) and f["loglik"][0] >= r["loglik"][-1] - 1e-9 * abs(r["loglik"][-1])


def test_train_gmm_diag_recovers_a_separated_model(vc, dr):
    """init="kmeans", n_init=1 on 20 000 frames of three mixtures 20 standard deviations apart: the fit converges and every
    mean lies within 6 standard errors of the sample mean of its own frames (tests/test_em_diag_host.py checks the same input
    with a numpy EM; a correct fit deviates by far less, because the mixtures do not overlap)."""
    Xh, lab, mu_true, sd = dr.recovery_case()
    r = vc.train_gmm(dev(Xh), n_components=3, n_init=1, init="kmeans", covariance_type="diag")
    assert r["converged"] and r["covars"].shape == (4, 3) and r["covariance_type"] == "diag"
    worst = dr.recovery_worst_deviation(Xh, lab, mu_true, r["means"])
    print(f"  {len(r['loglik'])} iterations, worst mean deviation {worst:.3g} standard errors")
    assert worst <= 6.0
    assert np.all(r["covars"] > 0) and abs(r["weights"].sum() - 1.0) < 1e-12


def test_train_gmm_diag_from_the_subsample_initialisation(vc, dr):
    """init="subsample" takes the variances from the same subsample as the means: the diagonal of its covariance."""
    Xh, lab, mu_true, sd = dr.recovery_case()
    a = vc.train_gmm(dev(Xh), n_components=3, n_init=2, n_iter=30, covariance_type="diag", seed=3)
    b = vc.train_gmm(dev(Xh), n_components=3, n_init=2, n_iter=30, covariance_type="diag", seed=3)
    assert a["covars"].shape == (4, 3) and np.all(a["covars"] > 0) and np.isfinite(a["loglik"]).all()
    assert np.array_equal(a["means"], b["means"]) and a["loglik"] == b["loglik"]


def test_train_gmm_defaults_are_the_full_covariance_fit(vc):
    w, mu, var = diag_model(71, 4, 16, spread=6.0)
    X = dev(draw(6, w, mu, var, 4000))
    r = vc.train_gmm(X)
    assert set(r) == {"weights", "means", "covars", "n_components", "loglik", "converged"}
    assert r["covars"].shape == (4, 4, 16) and r["means"].shape == (4, 16) and r["n_components"] == 16
    with pytest.raises(ValueError, match="covariance_type"):
        vc.train_gmm(X, covariance_type="spherical")


# ------------------------------------------------------------------------------------------------ 6. diag and full agree
def test_diagonal_and_full_estep_agree_on_a_diagonal_model(vc):
    Dj, M, N = 16, 4, 5000
    w, mu, var = diag_model(81, Dj, M, spread=1.5)
    X = dev(draw(7, w, mu, var, N))
    d0, d1, d2, dll = vc.unpack_stats(vc.estep_diag_dev(X, w, mu, var).cpu().numpy(), Dj, M)
    f0, f1, f2, fll = vc.unpack_full_stats(vc.estep_full_dev(X, w, mu, vc.expand_diag(var)).cpu().numpy(), Dj, M)
    f2d = np.stack([np.diag(f2[:, :, m]) for m in range(M)], axis=1)
    e = per_mixture_err((f0, f1, f2d), (d0, d1, d2))
    print(f"  full against diagonal: {e.max():.2e}, loglik {abs(fll - dll) / abs(dll):.2e}")
    assert e.max() <= TOL, e
    assert abs(fll - dll) <= TOL * abs(dll)


# ------------------------------------------------------------------------------------------------ 7. two ranks
def _two_rank_case():
    Dj, M, N = 16, 3, 8192
    w, mu, var = diag_model(91, Dj, M, spread=2.0, var_lo=0.1)
    return Dj, M, N, draw(8, w, mu, var, N), diag_model(92, Dj, M, spread=2.0, var_lo=0.1)


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import dist as vd

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    Dj, M, N, X, start = _two_rank_case()
    lo, hi = vd.shard_range(N, rank, world)
    r = vc.train_gmm(torch.from_numpy(X[lo:hi]).cuda().t(), n_components=M, n_iter=3, tol=0.0, refine=start, covariance_type="diag")
    q.put((rank, {k: r[k] for k in ("weights", "means", "covars", "loglik")}))
    dist.destroy_process_group()


def test_two_rank_train_gmm_diag_matches_single_process(vc):
    """Two gloo ranks on the one GPU, half of 8192 frames each, one all-reduce of the packed statistics per iteration: the
    parameters match the single-process fit to 1e-12 relative (sums taken in a different order), both ranks hold the same bits."""
    import queue
    import torch
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 90)
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
    ref = vc.train_gmm(torch.from_numpy(X).cuda().t(), n_components=M, n_iter=3, tol=0.0, refine=start, covariance_type="diag")
    for rank in (0, 1):
        for k in ("weights", "means", "covars"):
            err = np.max(np.abs(res[rank][k] - ref[k])) / np.max(np.abs(ref[k]))
            print(f"  rank {rank} {k}: {err:.2e}")
            assert err <= 1e-12, (rank, k, err)
        assert np.allclose(res[rank]["loglik"], ref["loglik"], rtol=1e-12, atol=0)
    for k in ("weights", "means", "covars"):
        assert np.array_equal(res[0][k], res[1][k])
    assert res[0]["loglik"] == res[1]["loglik"]
