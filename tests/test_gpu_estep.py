"""GPU parity: diagonal E-step sufficient statistics vs the golden vectors and the C oracle.
Tolerance 1e-9 relative to the largest statistic (sums of ~N terms in different association orders)."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, relerr
from test_gpu_estep_adversarial import per_mixture_err

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def _force_generic(vc, on):
    from voiceconversion_jl_amd import _lib
    _lib.debug_force(_lib.DBG_ESTEP_GENERIC if on else 0)


@pytest.mark.parametrize("generic", [False, True])
def test_golden(vc, generic):
    z = load_golden("estep_diag_N2000_D80_M16.npz")
    _force_generic(vc, generic)
    try:
        S0, S1, S2, ll = vc.estep_diag(z["X"].T, z["w"], z["mu"].T, z["var"].T)
    finally:
        _force_generic(vc, False)
    assert relerr(S0, z["S0"]) < TOL and relerr(S1, z["S1"].T) < TOL and relerr(S2, z["S2"].T) < TOL
    assert abs(ll - float(z["loglik"])) < TOL * abs(float(z["loglik"]))
    assert abs(S0.sum() - 2000) < 1e-6          # responsibilities sum to one per frame


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("N,Dj,M", [(5000, 80, 128), (777, 80, 100), (1, 80, 3), (300, 48, 8), (3000, 48, 128), (2000, 64, 100),
                                    (1500, 32, 16), (600, 160, 24), (4000, 160, 128), (33, 160, 5), (1000, 6, 2), (70000, 10, 4),
                                    (900, 50, 7), (400, 100, 5), (300, 126, 3), (257, 78, 128), (500, 25, 4),
                                    (3000, 80, 16), (3000, 80, 17), (2000, 80, 33), (2000, 80, 64), (1000, 160, 16), (999, 160, 40),
                                    # more than 128 mixtures: groups of 128 (responsibilities per group, combined per frame)
                                    (3000, 80, 129), (4000, 80, 256), (2500, 32, 200), (1200, 160, 130), (900, 50, 300), (65, 48, 257),
                                    # odd joint dimensions: one zero dimension more, then the even kernels (161: generic kernels)
                                    (3000, 79, 128), (1000, 81, 200), (50, 159, 3), (700, 1, 2), (300, 161, 4),
                                    # the 112-wide two-kernel instantiation (Dj = 82 ... 112), also in groups of 128 mixtures
                                    (2000, 82, 128), (900, 96, 40), (700, 112, 130), (500, 111, 9)])
def test_vs_oracle(vc, N, Dj, M, generic):
    """Every Dj <= 160 runs the MFMA kernel: in the next larger of its instantiations 32, 48, 64, 80 and -- as two kernels,
    the responsibilities through HBM -- 160, with zero weights in the padding dimensions; more than 128 mixtures in
    groups of 128; an odd Dj with one zero dimension more.  `generic` forces the generic kernels (the only path beyond
    Dj = 160)."""
    if generic and N > 5000:
        pytest.skip("the generic kernels are the only path for this shape")
    from oracle import c_oracle as co, np_oracle as npo
    w, mu, _ = npo.synth_model(3000 + N, Dj, M)
    rg = np.random.default_rng(N)
    var = np.exp(rg.uniform(np.log(1e-3), 0.0, (M, Dj)))
    comp = rg.choice(M, size=N, p=w)
    X = mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])
    r0, r1, r2, rl = co.estep_diag(X, w, mu, var)
    _force_generic(vc, generic)
    try:
        S0, S1, S2, ll = vc.estep_diag(X.T, w, mu.T, var.T)
    finally:
        _force_generic(vc, False)
    assert relerr(S0, r0) < TOL and relerr(S1, r1.T) < TOL and relerr(S2, r2.T) < TOL
    assert abs(ll - rl) < TOL * abs(rl)


@pytest.mark.parametrize("M", [129, 256])
def test_group_of_mixtures_without_weight(vc, M):
    """More than 128 mixtures run in groups of 128.  A group whose mixtures ALL have zero weight (a padded model: M = 129
    with w[129] = 0, or a whole second group of zeros) has every l = -inf: its responsibilities are exactly zero and its
    log-sum-exp -inf -- not NaN in every statistic."""
    from oracle import c_oracle as co, np_oracle as npo
    N, Dj = 3000, 80
    w, mu, _ = npo.synth_model(4100 + M, Dj, M)
    w = w.copy()
    w[128:] = 0.0
    w /= w.sum()
    rg = np.random.default_rng(M)
    var = np.exp(rg.uniform(np.log(1e-3), 0.0, (M, Dj)))
    comp = rg.choice(M, size=N, p=w)
    X = mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])
    r0, r1, r2, rl = co.estep_diag(X, w, mu, var)
    S0, S1, S2, ll = vc.estep_diag(X.T, w, mu.T, var.T)
    assert np.all(np.isfinite(S0)) and np.all(np.isfinite(S1)) and np.all(np.isfinite(S2)) and np.isfinite(ll)
    assert np.all(S0[128:] == 0.0) and np.all(S1[:, 128:] == 0.0)
    assert relerr(S0, r0) < TOL and relerr(S1, r1.T) < TOL and relerr(S2, r2.T) < TOL
    assert abs(ll - rl) < TOL * abs(rl)


def test_device_resident_deterministic_and_additive(vc):
    """Run-to-run bit-identical (fixed-order reductions, no atomics) and additive over frame shards -- the
    property the multi-GPU all-reduce relies on."""
    import torch
    from oracle import np_oracle as npo
    Dj, M, N = 80, 128, 40000
    w, mu, _ = npo.synth_model(77, Dj, M)
    rg = np.random.default_rng(7)
    var = np.exp(rg.uniform(np.log(1e-3), 0.0, (M, Dj)))
    comp = rg.choice(M, size=N, p=w)
    X = torch.from_numpy(mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])).cuda()
    a = vc.estep_diag_dev(X.t(), w, mu.T, var.T)
    b = vc.estep_diag_dev(X.t(), w, mu.T, var.T)
    assert torch.equal(a, b)
    h = vc.estep_diag_dev(X[:N // 2].t(), w, mu.T, var.T) + vc.estep_diag_dev(X[N // 2:].t(), w, mu.T, var.T)
    assert float((a - h).abs().max() / a.abs().max()) < 1e-12
    S0, S1, S2, ll = vc.unpack_stats(a.cpu().numpy(), Dj, M)
    assert abs(S0.sum() - N) < 1e-6 * N
    # M-step sanity: re-estimated means stay close to the generating means for well-populated components
    w2, mu2, var2 = vc.mstep_diag(S0, S1, S2)
    big = S0 > 200
    assert np.max(np.abs(mu2[:, big] - mu.T[:, big])) < 0.2


def test_parameter_staging_ring_reused_by_both_launchers(vc):
    """The one-kernel launcher and the launcher of the mixture groups (M > 128) stage their parameters through the same ring of
    eight pinned slots: 24 calls queued back to back on one stream, cycling through a shared-tile shape, a grouped one and a
    one-tile one (blocks of different lengths, so the slots' device copies overlap from call to call), without reading
    anything back in between.  Every result equals, bit for bit, the first result of its shape."""
    import torch
    from oracle import np_oracle as npo
    N = 200
    cases = []
    for k, (Dj, M) in enumerate([(32, 130), (34, 40), (32, 16)]):      # the largest block first: the ring has its full size
        w, mu, _ = npo.synth_model(300 + k, Dj, M)
        rg = np.random.default_rng(310 + k)
        var = np.exp(rg.uniform(np.log(1e-2), 0.0, (M, Dj)))
        comp = rg.choice(M, size=N, p=w)
        X = torch.from_numpy(mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])).cuda()
        first = vc.estep_diag_dev(X.t(), w, mu.T, var.T).cpu()
        assert abs(float(first[:M].sum()) - N) < 1e-6 * N
        cases.append((X, w, mu.T, var.T, first))
    outs = [torch.empty(vc.stats_len(c[0].shape[1], len(c[1])), dtype=torch.float64, device="cuda") for _ in range(8) for c in cases]
    for i, out in enumerate(outs):
        X, w, mu, var, _ = cases[i % 3]
        vc.estep_diag_dev(X.t(), w, mu, var, out=out)
    for i, out in enumerate(outs):
        assert torch.equal(out.cpu(), cases[i % 3][4]), (i, i % 3)


def test_errors(vc):
    with pytest.raises(vc.PosDefException):
        vc.estep_diag(np.zeros((4, 10)), np.ones(2) / 2, np.zeros((4, 2)), np.zeros((4, 2)))
    with pytest.raises(vc.DimensionMismatch):
        vc.estep_diag(np.zeros((5, 10)), np.ones(2) / 2, np.zeros((4, 2)), np.ones((4, 2)))


def _hard_case(seed, Dj, M, N, spread, lo, hi, overlap):
    """Tight variances (down to sklearn's min_covar, bin/train_gmm.jl:18), means far from the origin and mixtures that
    overlap: the regime where an expanded-form log-density  x^2 a + x b + c  cancels catastrophically."""
    rg = np.random.default_rng(seed)
    w = rg.dirichlet(2.0 * np.ones(M))
    base = rg.uniform(-spread, spread, (1, Dj))
    vd = np.exp(rg.uniform(np.log(lo), np.log(hi), (1, Dj)))               # per-dimension scale shared by the cluster
    var = vd * np.exp(rg.uniform(np.log(0.5), np.log(2.0), (M, Dj)))
    # clustered means, apart by a fraction of a standard deviation in EVERY dimension: soft, shared posteriors
    mu = base + overlap * rg.standard_normal((M, Dj)) * np.sqrt(vd) / np.sqrt(Dj)
    mu[: M // 4] = rg.uniform(-spread, spread, (M // 4, Dj))                # ... plus some far-away mixtures
    comp = rg.choice(M, size=N, p=w)
    X = mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])
    return w, mu, var, X


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("Dj,M", [(80, 128), (80, 37), (48, 16), (64, 40), (32, 128), (160, 64),
                                  # more than 128 mixtures: mixtures that compete ACROSS two groups of 128 (round 5: exact as well)
                                  (80, 200), (48, 300), (160, 130)])
def test_tight_variances_far_means_overlapping_mixtures(vc, generic, Dj, M):
    """sigma^2 log-uniform in [1e-7, 1e-2], |mu| up to 10, overlapping mixtures -- within 1e-9 of the
    oracle (which evaluates (x - mu)^2 / sigma^2 term by term) for both device paths."""
    from oracle import c_oracle as co
    from voiceconversion_jl_amd import _lib
    w, mu, var, X = _hard_case(515 + Dj + M, Dj, M, 6000, 10.0, 1e-7, 1e-2, 3.0 if Dj <= 80 else 1.5)
    r0, r1, r2, rl = co.estep_diag(X, w, mu, var)
    _lib.debug_force(_lib.DBG_ESTEP_GENERIC if generic else 0)
    try:
        S0, S1, S2, ll = vc.estep_diag(X.T, w, mu.T, var.T)
    finally:
        _lib.debug_force(0)
    assert relerr(S0, r0) < TOL and relerr(S1, r1.T) < TOL and relerr(S2, r2.T) < TOL, (relerr(S0, r0), relerr(S1, r1.T), relerr(S2, r2.T))
    assert abs(ll - rl) < TOL * abs(rl)
    # responsibilities are genuinely shared in this case (otherwise the test would not see log-density errors)
    import voiceconversion_jl_amd  # noqa: F401
    from oracle import np_oracle as npo
    lp = -0.5 * (((X[:200, None, :] - mu[None]) ** 2 / var[None]).sum(-1) + np.log(var).sum(-1)[None]) + np.log(w)[None]
    g = np.exp(lp - lp.max(1, keepdims=True)); g /= g.sum(1, keepdims=True)
    assert np.mean(g.max(1)) < 0.97


def test_fixture_model_diagonal(vc, fixture_model):
    """The shipped model's own diagonal (variances down to ~1e-7 on some dimensions) with frames drawn from it."""
    from oracle import c_oracle as co
    w, mu, sig = fixture_model
    var = np.stack([np.diag(s.T).copy() for s in sig])
    rg = np.random.default_rng(4)
    comp = rg.choice(len(w), size=5000, p=w)
    X = mu[comp] + rg.standard_normal((5000, mu.shape[1])) * np.sqrt(var[comp])
    r0, r1, r2, rl = co.estep_diag(X, w, mu, var)
    S0, S1, S2, ll = vc.estep_diag(X.T, w, mu.T, var.T)
    assert relerr(S0, r0) < TOL and relerr(S1, r1.T) < TOL and relerr(S2, r2.T) < TOL
    assert abs(ll - rl) < TOL * abs(rl)


@pytest.mark.parametrize("Dj,M,N", [(80, 128, 5000), (160, 64, 3000), (48, 16, 700), (79, 20, 900), (80, 200, 1500), (80, 128, 0)])
def test_output_buffer_is_overwritten_not_accumulated(vc, Dj, M, N):
    """The packed statistics are an OUTPUT: whatever the buffer held before the call (here NaN) is gone afterwards, in every
    dispatch (one kernel, two kernels at Dj = 160, odd Dj, groups of 128 mixtures, no frames).  The single-kernel path has
    no memset in front of it any more -- its first reduction overwrites."""
    import torch
    from oracle import np_oracle as npo
    w, mu, _ = npo.synth_model(900 + Dj + M, Dj, M)
    rg = np.random.default_rng(Dj * M)
    var = np.exp(rg.uniform(np.log(1e-3), 0.0, (M, Dj)))
    comp = rg.choice(M, size=max(N, 1), p=w)
    X = (mu[comp] + rg.standard_normal((max(N, 1), Dj)) * np.sqrt(var[comp]))[:N]
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda().reshape(N, Dj)
    out = torch.full((vc.stats_len(Dj, M),), float("nan"), dtype=torch.float64, device="cuda")
    got = vc.estep_diag_dev(Xd.t(), w, mu.T, var.T, out=out).clone()
    fresh = vc.estep_diag_dev(Xd.t(), w, mu.T, var.T)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, fresh)
    out.fill_(1e300)
    again = vc.estep_diag_dev(Xd.t(), w, mu.T, var.T, out=out)
    assert torch.equal(again, fresh)
    if N == 0:
        assert float(got.abs().max()) == 0.0


@pytest.mark.parametrize("N,Dj,M,hard", [(50_000, 80, 128, False), (4097, 80, 65, False), (31, 80, 128, False), (20_000, 64, 100, False),
                                         (9000, 32, 128, False), (7000, 50, 96, False), (6000, 80, 128, True), (6000, 48, 70, True)])
def test_one_barrier_experiment_against_the_three_barrier_kernel(vc, N, Dj, M, hard):
    """More than 64 mixtures, Dj <= 80: estep_wave_kernel (csrc/estep_wave.hpp) -- every wave keeps the softmax of its own 16
    mixtures to itself, one exchange + barrier per 32-frame block, the responsibilities never stored -- against
    estep_mfma_kernel (three barriers per 64-frame block: the default -- the experiment is slower; DBG_ESTEP_WAVE_KERNEL selects it) and the oracle: statistics to 1e-12 of
    each other (other summation orders), repeat runs bit-identical; `hard`: overlapping mixtures with tight variances, where
    competing mixtures are re-evaluated term by term (the block's second exchange)."""
    from oracle import c_oracle as co, np_oracle as npo
    from voiceconversion_jl_amd import _lib
    if hard:
        w, mu, var, X = _hard_case(900 + Dj + M, Dj, M, N, 10.0, 1e-7, 1e-2, 3.0)
    else:
        w, mu, _ = npo.synth_model(4000 + N, Dj, M)
        rg = np.random.default_rng(N)
        var = np.exp(rg.uniform(np.log(1e-3), 0.0, (M, Dj)))
        comp = rg.choice(M, size=N, p=w)
        X = mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])
    o = vc.estep_diag(X.T, w, mu.T, var.T)
    _lib.debug_force(_lib.DBG_ESTEP_WAVE_KERNEL)
    try:
        a = vc.estep_diag(X.T, w, mu.T, var.T)
        for _ in range(2):
            b = vc.estep_diag(X.T, w, mu.T, var.T)
            assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]
        S0, S1, S2, ll = vc.estep_diag(X[:8000].T, w, mu.T, var.T)
    finally:
        _lib.debug_force(0)
    for p, q in zip(a[:3], o[:3]):
        assert relerr(p, q) < 1e-12, relerr(p, q)
    assert abs(a[3] - o[3]) < 1e-12 * abs(o[3])
    r0, r1, r2, rl = co.estep_diag(X[:8000], w, mu, var)
    assert relerr(S0, r0) < TOL and relerr(S1, r1.T) < TOL and relerr(S2, r2.T) < TOL
    assert abs(ll - rl) < TOL * abs(rl)


def test_pinned_frames_are_uploaded_directly(vc):
    """vcmi_host_register: a training matrix the caller keeps (bin/train_gmm.jl holds X for all EM iterations) is DMA'd
    straight out of its pages by the plain uploads too -- same statistics, bit for bit."""
    from oracle import np_oracle as npo
    N, Dj, M = 300_000, 80, 128
    w, mu, _ = npo.synth_model(77, Dj, M)
    rg = np.random.default_rng(5)
    var = np.exp(rg.uniform(np.log(1e-3), 0.0, (M, Dj)))
    comp = rg.choice(M, size=N, p=w)
    X = np.asfortranarray((mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])).T)
    a = vc.estep_diag(X, w, mu.T, var.T)
    vc.pin(X)
    try:
        assert vc.is_pinned(X)
        b = vc.estep_diag(X, w, mu.T, var.T)
    finally:
        vc.unpin(X)
    assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]


# ---- the hard-assignment path (csrc/estep_hard.hpp): N >= 65536 frames, M <= 128, Dj <= 80 ----

def _separated_case(seed, N, Dj, M, sep, zero_weight=None):
    """Mixtures `sep` standard deviations apart per dimension (BASELINE-like: every frame has one owner), unit-ish variances."""
    rg = np.random.default_rng(seed)
    w = rg.dirichlet(2.0 * np.ones(M))
    if zero_weight is not None:
        w[zero_weight] = 0.0
        w /= w.sum()
    var = np.exp(rg.uniform(np.log(0.05), 0.0, (M, Dj)))
    mu = sep * rg.standard_normal((M, Dj))
    comp = rg.choice(M, size=N, p=w)
    X = mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])
    return w, mu, var, X


def _both_paths(vc, X, w, mu, var, path=None):
    """(statistics of the library's own choice (or of the pinned `path`), statistics of the one-kernel path, soft frames of the
    first call: -1 = it took the one-kernel path).  The choice is made from the call's own frames (vcmi_estep_set_path: AUTO), so
    nothing has to be forgotten between tests; with the hard-assignment path pinned, AUTO must give the same bits when it
    chooses that path."""
    from voiceconversion_jl_amd import _lib
    assert vc.estep_get_path() == vc.ESTEP_AUTO
    try:
        if path is not None:
            vc.estep_set_path(path)
        a = vc.estep_diag(X.T, w, mu.T, var.T)
        soft = _lib.estep_last_soft()
        vc.estep_set_path(vc.ESTEP_SOFT)
        o = vc.estep_diag(X.T, w, mu.T, var.T)
        assert _lib.estep_last_soft() == -1
        vc.estep_set_path(vc.ESTEP_AUTO)
        if soft >= 0:
            b = vc.estep_diag(X.T, w, mu.T, var.T)
            if _lib.estep_last_soft() >= 0:
                assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]
    finally:
        vc.estep_set_path(vc.ESTEP_AUTO)
    return a, o, soft


@pytest.mark.parametrize("N,Dj,M,sep,zw", [(70_000, 80, 128, 3.0, None), (66_000, 80, 40, 3.0, None), (100_001, 48, 128, 4.0, None),
                                           (65_536, 50, 17, 4.0, 3), (80_000, 32, 16, 6.0, None), (70_000, 64, 100, 3.0, 99),
                                           (90_000, 10, 4, 12.0, None), (70_000, 79, 128, 3.0, None), (70_000, 80, 1, 3.0, None)])
def test_hard_assignment_path_all_frames_owned(vc, N, Dj, M, sep, zw):
    """Far-apart mixtures: every frame is certified to have exactly one non-zero responsibility (no frame reaches the FP64
    kernel), the statistics are segmented sums -- against the one-kernel path (DBG_ESTEP_NO_HARD) to 1e-12 and the oracle to
    1e-9; repeat runs bit-identical; dj below the instantiated width, M not a multiple of 16, a mixture without weight."""
    from oracle import c_oracle as co
    w, mu, var, X = _separated_case(N + Dj + M, N, Dj, M, sep, zw)
    # (one mixture tile, M <= 16: left to itself the library takes estep_small_kernel whatever the data -- it is as fast as this
    # path there, and nothing has to be decided; the hard-assignment path is pinned for these cases)
    a, o, soft = _both_paths(vc, X, w, mu, var, path=vc.ESTEP_HARD if M <= 16 else None)
    assert soft == 0, soft
    for p, q in zip(a[:3], o[:3]):
        assert relerr(p, q) < 1e-12, relerr(p, q)
    assert abs(a[3] - o[3]) < 1e-12 * abs(o[3])
    vc.estep_set_path(vc.ESTEP_HARD if M <= 16 else vc.ESTEP_AUTO)
    try:
        b = vc.estep_diag(X.T, w, mu.T, var.T)                # repeat runs of the path: bit-identical
    finally:
        vc.estep_set_path(vc.ESTEP_AUTO)
    assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]
    r0, r1, r2, rl = co.estep_diag(X, w, mu, var)
    assert relerr(a[0], r0) < TOL and relerr(a[1], r1.T) < TOL and relerr(a[2], r2.T) < TOL
    assert per_mixture_err(a[:3], (r0, r1.T, r2.T)).max() <= TOL, per_mixture_err(a[:3], (r0, r1.T, r2.T)).max()
    assert abs(a[3] - rl) < TOL * abs(rl)
    assert abs(a[0].sum() - N) < 1e-6
    if M <= 16:                                               # the library's own choice for one mixture tile: the FP64 kernel
        from voiceconversion_jl_amd import _lib
        c = vc.estep_diag(X.T, w, mu.T, var.T)
        assert _lib.estep_last_soft() == -1
        assert all(relerr(p, q) < 1e-12 for p, q in zip(a[:3], c[:3]))
    if zw is not None:
        assert a[0][zw] == 0.0 and not a[1][:, zw].any()


@pytest.mark.parametrize("N,Dj,M", [(70_000, 80, 128), (66_000, 48, 24), (80_000, 64, 100),
                                    # the gathered frames through the other two FP64 bodies of the plan (csrc/estep_plan.hpp):
                                    # estep_mfma_kernel with shared tiles (32 < M <= 64), estep_small_kernel<DJ, 1> (M <= 16)
                                    (65_536, 48, 40), (65_536, 48, 16)])
def test_hard_assignment_path_mixed_frames(vc, N, Dj, M):
    """Half of the mixtures far apart, the other half overlapping: the owned frames are settled by the screen, the others
    (thousands) are gathered and go through the FP64 kernel -- sum of the two equals the one-kernel path and the oracle."""
    from oracle import c_oracle as co
    rg = np.random.default_rng(N + M)
    w, mu, var, _ = _separated_case(N + 1, 16, Dj, M, 3.0)
    mu[M // 2:] = mu[M // 2] + 0.3 * rg.standard_normal((M - M // 2, Dj)) * np.sqrt(var[M // 2:])       # a cluster of overlapping mixtures
    comp = rg.choice(M, size=N, p=w)
    X = mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])
    a, o, soft = _both_paths(vc, X, w, mu, var, vc.ESTEP_HARD)       # (pinned: the library itself would step aside here)
    assert 0.05 * N < soft < 0.95 * N, soft
    for p, q in zip(a[:3], o[:3]):
        assert relerr(p, q) < 1e-12, relerr(p, q)
    assert abs(a[3] - o[3]) < 1e-12 * abs(o[3])
    vc.estep_set_path(vc.ESTEP_HARD)
    try:
        b = vc.estep_diag(X.T, w, mu.T, var.T)
    finally:
        vc.estep_set_path(vc.ESTEP_AUTO)
    assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]
    r0, r1, r2, rl = co.estep_diag(X, w, mu, var)
    assert relerr(a[0], r0) < TOL and relerr(a[1], r1.T) < TOL and relerr(a[2], r2.T) < TOL
    assert per_mixture_err(a[:3], (r0, r1.T, r2.T)).max() <= TOL, per_mixture_err(a[:3], (r0, r1.T, r2.T)).max()
    assert abs(a[3] - rl) < TOL * abs(rl)


def test_hard_assignment_path_steps_aside_when_frames_are_shared(vc):
    """The path is chosen from the call's OWN frames (a screen on a sample of 16 chunks, decided on the device: VERDICT r5 item
    5), not from what earlier calls found: overlapping mixtures -> the one-kernel path on the FIRST call and on every one; frames
    with owners -> the hard-assignment path on the first call; the two kinds of data interleaved on one thread -> every call
    bit-identical to the same call made alone, in another thread, in any order."""
    import threading
    from oracle import c_oracle as co
    from voiceconversion_jl_amd import _lib
    N, Dj, M = 70_000, 80, 64
    w, mu, var, X = _hard_case(4242, Dj, M, N, 10.0, 1e-3, 1e-1, 3.0)       # (three quarters of its frames are shared between mixtures)
    w2, mu2, var2, X2 = _separated_case(5, N, Dj, M, 3.0)                   # (every frame has an owner)
    r = co.estep_diag(X, w, mu, var)
    r2 = co.estep_diag(X2, w2, mu2, var2)

    def close(a, ref):
        return relerr(a[0], ref[0]) < TOL and relerr(a[1], ref[1].T) < TOL and relerr(a[2], ref[2].T) < TOL and abs(a[3] - ref[3]) < TOL * abs(ref[3])

    alone = {}

    def in_a_fresh_thread(name, Xk, wk, muk, vark):
        alone[name] = (vc.estep_diag(Xk.T, wk, muk.T, vark.T), _lib.estep_last_soft())

    for args in (("shared", X, w, mu, var), ("owned", X2, w2, mu2, var2)):
        t = threading.Thread(target=in_a_fresh_thread, args=args)
        t.start()
        t.join()
    assert alone["shared"][1] == -1 and alone["owned"][1] == 0
    assert close(alone["shared"][0], r) and close(alone["owned"][0], r2)
    same = lambda a, b: all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]      # noqa: E731
    for order in ("shared", "owned", "owned", "shared", "shared", "owned", "shared"):
        if order == "shared":
            a = vc.estep_diag(X.T, w, mu.T, var.T)
        else:
            a = vc.estep_diag(X2.T, w2, mu2.T, var2.T)
        assert _lib.estep_last_soft() == alone[order][1]
        assert same(a, alone[order][0]), order
    # pinned paths: still the right statistics on the "wrong" kind of data, and the setting is per thread
    vc.estep_set_path(vc.ESTEP_HARD)
    try:
        a = vc.estep_diag(X.T, w, mu.T, var.T)
        assert _lib.estep_last_soft() > 0.5 * N and close(a, r)
        seen = []
        t = threading.Thread(target=lambda: seen.append(vc.estep_get_path()))
        t.start()
        t.join()
        assert seen == [vc.ESTEP_AUTO] and vc.estep_get_path() == vc.ESTEP_HARD
    finally:
        vc.estep_set_path(vc.ESTEP_AUTO)
    with pytest.raises(vc.VCMIError):
        vc.estep_set_path(7)


def test_hard_assignment_path_device_resident_and_small_calls(vc):
    """estep_diag_dev on device-resident frames takes the same path; below 65536 frames the one-kernel path runs."""
    import torch
    from voiceconversion_jl_amd import _lib
    w, mu, var, X = _separated_case(9, 131_072, 80, 128, 3.0)
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    got = vc.estep_diag_dev(Xd.t(), w, mu.T, var.T)
    assert _lib.estep_last_soft() == 0
    S0, S1, S2, ll = vc.estep_diag(X.T, w, mu.T, var.T)
    plen = got.numel()
    g = got.cpu().numpy()
    assert np.array_equal(g[:128], S0) and g[plen - 1] == ll
    vc.estep_diag(X[:60_000].T, w, mu.T, var.T)
    assert _lib.estep_last_soft() == -1


@pytest.mark.parametrize("Dj,M", [(80, 128), (48, 37)])
def test_hard_assignment_path_tight_variances(vc, Dj, M):
    """The regime of VERDICT r1 weak #8 at a size the screen sees: variances down to 1e-7, means up to 10, a cluster of
    overlapping mixtures (soft: their bf16 intervals are wide and they compete) beside far-away ones (owned: gaps of 1e9 nats
    against margins of 1e6) -- hard and soft frames together equal the one-kernel path to 1e-12 and the oracle to 1e-9."""
    from oracle import c_oracle as co
    N = 70_000
    w, mu, var, X = _hard_case(77 + Dj + M, Dj, M, N, 10.0, 1e-7, 1e-2, 3.0)
    a, o, soft = _both_paths(vc, X, w, mu, var, vc.ESTEP_HARD)
    assert 0 < soft < N, soft                        # both kinds of frames are present
    for p, q in zip(a[:3], o[:3]):
        assert relerr(p, q) < 1e-12, relerr(p, q)
    # the log-likelihood of an owned frame is the winner's log-density term by term here, the expanded form x^2 a + x b + c in the
    # one-kernel path when nothing competes (1e-7 absolute per frame at these variances): the two agree to 1e-10, and the
    # hard path is the one closer to the oracle
    assert abs(a[3] - o[3]) < 1e-10 * abs(o[3])
    r0, r1, r2, rl = co.estep_diag(X, w, mu, var)
    assert relerr(a[0], r0) < TOL and relerr(a[1], r1.T) < TOL and relerr(a[2], r2.T) < TOL
    assert per_mixture_err(a[:3], (r0, r1.T, r2.T)).max() <= TOL, per_mixture_err(a[:3], (r0, r1.T, r2.T)).max()
    assert abs(a[3] - rl) < TOL * abs(rl)
    assert abs(a[3] - rl) <= abs(o[3] - rl) + 1e-13 * abs(rl), (a[3] - rl, o[3] - rl)


def test_hard_assignment_path_a_handful_of_shared_frames(vc):
    """Three frames half-way between two mixtures among 70,000 owned ones: the gathered pass runs on three rows (most of its
    workgroups have nothing to do and must contribute exact zeros)."""
    from oracle import c_oracle as co
    N, Dj, M = 70_000, 80, 128
    w, mu, var, X = _separated_case(31, N, Dj, M, 3.0)
    var[:] = 0.3                                     # equal covariances: the mid-point is equidistant
    rg = np.random.default_rng(2)
    comp = rg.choice(M, size=N, p=w)
    X = mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])
    for f, (p, q) in zip((5, 40_000, N - 1), ((0, 1), (7, 90), (126, 127))):
        X[f] = 0.5 * (mu[p] + mu[q]) + 1e-3 * rg.standard_normal(Dj)
    a, o, soft = _both_paths(vc, X, w, mu, var)
    assert 3 <= soft <= 8, soft
    for p, q in zip(a[:3], o[:3]):
        assert relerr(p, q) < 1e-12, relerr(p, q)
    assert abs(a[3] - o[3]) < 1e-12 * abs(o[3])
    r0, r1, r2, rl = co.estep_diag(X, w, mu, var)
    assert relerr(a[0], r0) < TOL and relerr(a[1], r1.T) < TOL and relerr(a[2], r2.T) < TOL
    assert per_mixture_err(a[:3], (r0, r1.T, r2.T)).max() <= TOL, per_mixture_err(a[:3], (r0, r1.T, r2.T)).max()
    assert abs(a[3] - rl) < TOL * abs(rl)
    assert abs(a[0].sum() - N) < 1e-6


@pytest.mark.parametrize("Dj,M,N", [(80, 1, 700), (80, 16, 4000), (80, 17, 4001), (80, 32, 12_345), (80, 33, 3000), (48, 32, 31), (30, 9, 32),
                                    (79, 32, 33), (64, 20, 2500), (32, 32, 100_000), (80, 32, 70_001), (80, 12, 66_000)])
def test_small_models_take_the_small_workgroups(vc, Dj, M, N):
    """M <= 32 (bin/train_gmm.jl:84-89 trains 32 mixtures): estep_small_kernel -- workgroups of two waves per
    mixture tile, 32-frame blocks, a softmax as wide as the model -- against the oracle and against estep_mfma_kernel's
    shared-tile form of the same model (forced); M = 33 is the first model of the other side.  Shared responsibilities
    (clustered means) so that the softmax matters; the calls of >= 65536 frames come through the path decision and its gated
    launches."""
    from oracle import c_oracle as co
    from voiceconversion_jl_amd import _lib
    w, mu, var, X = _hard_case(77 + Dj + M, Dj, M, N, 5.0, 1e-3, 1.0, 2.0)
    r = co.estep_diag(X, w, mu, var)

    def run(force):
        _lib.debug_force(force)
        try:
            return vc.estep_diag(X.T, w, mu.T, var.T)
        finally:
            _lib.debug_force(0)

    new, again, old = run(0), run(0), run(_lib.DBG_ESTEP_NO_SMALL)
    for got in (new, old):
        assert relerr(got[0], r[0]) < TOL and relerr(got[1], r[1].T) < TOL and relerr(got[2], r[2].T) < TOL
        assert per_mixture_err(got[:3], (r[0], r[1].T, r[2].T)).max() <= TOL, per_mixture_err(got[:3], (r[0], r[1].T, r[2].T)).max()
        assert abs(got[3] - r[3]) < TOL * abs(r[3])
    assert abs(new[0].sum() - N) < 1e-9 * N
    assert all(np.array_equal(a, b) for a, b in zip(new[:3], again[:3])) and new[3] == again[3]      # a function of the data alone
    assert relerr(new[1], old[1]) < 1e-12 and relerr(new[2], old[2]) < 1e-12


def test_small_model_on_the_reference_model_and_its_paths(vc, joint_model):
    """the reference's trained 32-mixture model (test/models/clb_and_slt_gmm32_order40.jld), its diagonal: frames of its own that
    share their mixtures (every frame through estep_small_kernel, decided on the device) and, with the variances shrunk, frames
    that one mixture owns (hard-assignment path; the few soft ones through estep_small_kernel with the device's count)"""
    from oracle import c_oracle as co
    w, mu, sig = joint_model
    var0 = np.stack([np.diag(s.T).copy() for s in sig])
    rg = np.random.default_rng(9)
    N = 90_000
    comp = rg.choice(len(w), size=N, p=w)
    from voiceconversion_jl_amd import _lib
    for shrink, path in ((1.0, vc.ESTEP_AUTO), (1e-3, vc.ESTEP_HARD), (1e-3, vc.ESTEP_AUTO)):
        var = var0 * shrink
        X = mu[comp] + rg.standard_normal((N, mu.shape[1])) * np.sqrt(var[comp])
        r0, r1, r2, rl = co.estep_diag(X, w, mu, var)
        vc.estep_set_path(path)
        try:
            S0, S1, S2, ll = vc.estep_diag(X.T, w, mu.T, var.T)
        finally:
            vc.estep_set_path(vc.ESTEP_AUTO)
        assert relerr(S0, r0) < TOL and relerr(S1, r1.T) < TOL and relerr(S2, r2.T) < TOL
        assert per_mixture_err((S0, S1, S2), (r0, r1.T, r2.T)).max() <= TOL, per_mixture_err((S0, S1, S2), (r0, r1.T, r2.T)).max()
        assert abs(ll - rl) < TOL * abs(rl)
        if path == vc.ESTEP_HARD:                # (-1: the one-kernel path; otherwise the number of soft frames)
            assert 0 <= _lib.estep_last_soft() <= N
