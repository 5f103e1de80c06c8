"""GPU: device k-means (csrc/kmeans.hip, kmeans.py) against the numpy restatement of tests/kmeans_restatement.py --
assignment (labels exact, distances of the direct difference), adversarial frames where |x|^2 - 2 x.c + |c|^2 loses
every digit, Lloyd from fixed centers iteration by iteration (with relocation of an empty cluster), k-means++ picks,
end-to-end determinism, train_gmm(init="kmeans"), two gloo ranks, and the error paths."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import kmeans_restatement as kr
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _vc():
    import voiceconversion_jl_amd as vc
    return vc, sys.modules["voiceconversion_jl_amd.kmeans"]


def dev(X):
    """(N,Dj) rows -> (Dj,N) dense device matrix."""
    return torch.from_numpy(np.ascontiguousarray(X)).cuda().t()


def run_assign(X, C):
    vc, km = _vc()
    N = len(X)
    st = km.KMeansState(X.shape[1], len(C), C.T)
    lab = torch.empty(N, dtype=torch.int32, device="cuda")
    stats = st.assign(dev(X), labels=lab).cpu().numpy()
    d2 = st.mind2(N, "cuda").cpu().numpy()
    return lab.cpu().numpy(), d2, stats


@pytest.mark.parametrize("Dj", [3, 24, 80, 81, 160, 200])
@pytest.mark.parametrize("M", [1, 7, 64, 128])
def test_assign_matches_restatement(Dj, M):
    rng = np.random.default_rng(Dj * 1000 + M)
    N = 3001
    X = rng.standard_normal((N, Dj)) + 2.0
    C = X[rng.choice(N, M, replace=False)] + 0.3 * rng.standard_normal((M, Dj))
    lab, d2, stats = run_assign(X, C)
    rl, rd = kr.assign(X, C)
    assert np.array_equal(lab, rl)
    assert np.max(np.abs(d2 - rd) / rd) <= 1e-13
    cnt = np.bincount(rl, minlength=M)
    assert np.array_equal(stats[:M], cnt.astype(float))
    S1 = stats[M:M + M * Dj].reshape(M, Dj)
    ref1 = np.array([X[rl == m].sum(0) for m in range(M)])
    assert np.max(np.abs(S1 - ref1)) <= 1e-12 * np.max(np.abs(X)) * N
    assert abs(stats[-1] - rd.sum()) <= 1e-12 * rd.sum()


@pytest.mark.parametrize("Dj", [5, 80, 200])
def test_assign_adversarial_ties_bisectors_and_cancellation(Dj):
    rng = np.random.default_rng(7 + Dj)
    M = 24
    # (1) exact ties: centers 3 and 17 differ only in dimension 1 (3.0 +- 0.5, exact), frames on the bisector x_1 = 3.0
    C = rng.standard_normal((M, Dj))
    C[17] = C[3]
    C[3, 1], C[17, 1] = 3.5, 2.5
    tie = np.repeat(C[3][None], 300, axis=0) + 0.01 * rng.standard_normal((300, Dj))
    tie[:, 1] = 3.0
    # (2) a few ulps either side of that bisector
    near = tie.copy()
    k = rng.integers(-4, 5, size=len(near))
    near[:, 1] = [np.nextafter(3.0, np.inf if s > 0 else -np.inf) if s else 3.0 for s in k]
    for i, s in enumerate(k):
        for _ in range(abs(int(s)) - 1):
            near[i, 1] = np.nextafter(near[i, 1], np.inf if s > 0 else -np.inf)
    X = np.vstack([tie, near])
    lab, d2, _ = run_assign(X, C)
    rl, rd = kr.assign(X, C)
    assert np.array_equal(lab, rl)
    assert np.all(lab[:300] == 3)                 # every exact tie goes to the smaller index
    assert np.array_equal(d2, rd)                 # same order and rounding: bit-identical distances
    # (3) mean 1e4 (and 1e6), spread 1e-2: the expanded form keeps few (no) correct digits
    for mean in (1e4, 1e6):
        Xc = mean + 1e-2 * rng.standard_normal((4000, Dj))
        Cc = Xc[rng.choice(4000, M, replace=False)] + 1e-3 * rng.standard_normal((M, Dj))
        lab, d2, _ = run_assign(Xc, Cc)
        rl, rd = kr.assign(Xc, Cc)
        if mean == 1e6:
            naive = np.argmin((Xc * Xc).sum(1)[:, None] - 2.0 * Xc @ Cc.T + (Cc * Cc).sum(1)[None], axis=1)
            assert np.any(naive != rl)            # (the data does defeat a GEMM + argmin)
        assert np.array_equal(lab, rl)
        assert np.max(np.abs(d2 - rd) / rd) <= 1e-13


@pytest.mark.parametrize("far", [False, True])
def test_lloyd_from_fixed_centers_matches_restatement_every_iteration(far):
    vc, km = _vc()
    rng = np.random.default_rng(11)
    Dj, M, N = 24, 16, 6000
    X = 3.0 * rng.standard_normal((12, Dj))[rng.integers(0, 12, N)] + rng.standard_normal((N, Dj))
    C0 = X[rng.choice(N, M, replace=False)].copy()
    if far:
        C0[5] = 1e3                                # far from every frame: empty at the first assignment -> relocated
    C, inertia, n_iter, lab, hist = kr.lloyd(X, C0, max_iter=50, tol_abs=0.0)
    Xd = dev(X)
    st = km.KMeansState(Dj, M, C0.T)
    stats = torch.empty(km.kmeans_stats_len(Dj, M), dtype=torch.float64, device="cuda")
    labels = torch.empty(N, dtype=torch.int32, device="cuda")
    relocated = 0
    for it, (rlab, rC, rin) in enumerate(hist):
        st.assign(Xd, labels=labels, out=stats)
        assert np.array_equal(labels.cpu().numpy(), rlab), f"iteration {it}"
        shift, inr, ne = st.update(stats)
        assert abs(inr - rin) <= 1e-12 * rin
        if ne:
            relocated += ne
            shift = st.relocate(stats, st.far(Xd, ne, 0))
        Cg = st.get().T
        assert np.max(np.abs(Cg - rC)) <= 1e-12 * np.max(np.abs(rC)), f"iteration {it}"
    assert relocated == (1 if far else 0)
    r = vc.kmeans(Xd, M, init=C0.T, max_iter=50, tol=0.0)
    assert r["n_iter"] == n_iter
    assert np.array_equal(r["labels"].cpu().numpy(), lab)
    assert np.max(np.abs(r["centers"].T - C)) <= 1e-12 * np.max(np.abs(C))
    assert abs(r["inertia"] - inertia) <= 1e-12 * inertia


@pytest.mark.parametrize("Dj,M", [(3, 8), (80, 64), (81, 7)])
def test_seeding_picks_match_restatement(Dj, M):
    vc, km = _vc()
    rng0 = np.random.default_rng(Dj + M)
    N = 5000
    X = rng0.standard_normal((N, Dj)) * rng0.uniform(0.5, 2.0, Dj)
    picks, margin = kr.kpp(X, M, np.random.default_rng(99))
    assert margin > 1e-9, "a target lies on a prefix boundary: choose another seed"
    st = km.KMeansState(Dj, M)
    km._seed(st, dev(X), M, np.random.default_rng(99), km._Comm(None), 0, N)
    Cg = st.get().T
    assert np.array_equal(Cg, X[picks])           # picks are frames of X, the same ones


def test_end_to_end_deterministic_and_recovers_partition():
    vc, _ = _vc()
    rng = np.random.default_rng(5)
    M, Dj = 10, 16
    mu = 8.0 * rng.standard_normal((M, Dj))
    comp = rng.integers(0, M, 20000)
    X = mu[comp] + 0.3 * rng.standard_normal((20000, Dj))
    Xd = dev(X)
    a = vc.kmeans(Xd, M, n_init=3, seed=4)
    b = vc.kmeans(Xd, M, n_init=3, seed=4)
    assert np.array_equal(a["centers"], b["centers"]) and a["inertia"] == b["inertia"]
    assert torch.equal(a["labels"], b["labels"])
    lab = a["labels"].cpu().numpy()
    for k in range(M):
        assert len(set(lab[comp == k])) == 1
    assert len(set(lab)) == M
    C, inertia, n_iter, rl = kr.kmeans(X, M, n_init=3, seed=4)
    assert np.array_equal(lab, rl) and a["n_iter"] == n_iter
    assert np.max(np.abs(a["centers"].T - C)) <= 1e-12 * np.max(np.abs(C))


def test_train_gmm_kmeans_init():
    vc, _ = _vc()
    import synthdata as sd
    from voiceconversion_jl_amd.train import data_covariance
    Dj, M, N = 8, 4, 12000
    w, mu, sig = sd.synth_model(31, Dj, M, lam_lo=1e-2)
    X = sd.sample_frames(32, w, 4.0 * mu, sig, N, 0, Dj)
    Xd = dev(X)
    cv = data_covariance(Xd)
    ref = np.cov(X.T)
    assert np.max(np.abs(cv - ref)) <= 1e-10 * np.max(np.abs(ref))
    r1 = vc.train_gmm(Xd, n_components=M, n_iter=30, n_init=1, tol=0.0, seed=3, init="kmeans")
    r2 = vc.train_gmm(Xd, n_components=M, n_iter=30, n_init=1, tol=0.0, seed=3, init="kmeans")
    ll = np.array(r1["loglik"])
    assert np.all(np.diff(ll) >= -1e-9 * np.abs(ll[1:]))
    assert np.array_equal(r1["means"], r2["means"]) and r1["loglik"] == r2["loglik"]
    # beats one Gaussian fitted to the same frames
    sign, logdet = np.linalg.slogdet(ref)
    Z = np.linalg.solve(np.linalg.cholesky(ref), (X - X.mean(0)).T)
    ll1 = np.mean(-0.5 * (Z * Z).sum(0)) - 0.5 * logdet - 0.5 * Dj * np.log(2 * np.pi)
    assert ll[-1] > ll1 + 0.1
    with pytest.raises(ValueError):
        vc.train_gmm(Xd, n_components=M, n_iter=1, init="other")


def test_errors():
    vc, km = _vc()
    X = np.random.default_rng(0).standard_normal((10, 4))
    with pytest.raises(vc.DimensionMismatch):
        vc.kmeans(dev(X), 11)
    with pytest.raises(vc.DimensionMismatch):
        vc.kmeans(torch.zeros((0, 10), dtype=torch.float64, device="cuda"), 2)
    with pytest.raises(vc.DimensionMismatch):
        km.KMeansState(257, 4)
    Xn = X.copy()
    Xn[3, 2] = np.nan
    with pytest.raises(vc.VCMIError):
        vc.kmeans(dev(Xn), 3, n_init=1)
    with pytest.raises(vc.VCMIError):
        vc.kmeans(dev(Xn), 3, init=X[:3].T)
    # the library still works after a refused input
    assert vc.kmeans(dev(X), 3, n_init=1)["centers"].shape == (4, 3)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import dist as vd

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    X, C0 = _dist_data()
    lo, hi = vd.shard_range(len(X), rank, world)
    Xd = torch.from_numpy(X[lo:hi]).cuda().t()
    r = vc.kmeans(Xd, C0.shape[0], init=C0.T, max_iter=40, tol=0.0)
    s = vc.kmeans(Xd, C0.shape[0], n_init=2, seed=8)
    q.put((rank, {"centers": r["centers"], "labels": r["labels"].cpu().numpy(), "n_iter": r["n_iter"],
                  "inertia": r["inertia"], "seeded": s["centers"]}))
    dist.destroy_process_group()


def _dist_data():
    rng = np.random.default_rng(21)
    Dj, M, N = 12, 9, 7001
    X = 2.0 * rng.standard_normal((15, Dj))[rng.integers(0, 15, N)] + rng.standard_normal((N, Dj))
    C0 = X[rng.choice(N, M, replace=False)].copy()
    C0[2] = 500.0                                      # relocation across ranks
    return X, C0


def test_two_rank_lloyd_matches_single_process():
    vc, _ = _vc()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 90)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    X, C0 = _dist_data()
    Xd = dev(X)
    r = vc.kmeans(Xd, C0.shape[0], init=C0.T, max_iter=40, tol=0.0)
    assert np.array_equal(np.concatenate([res[0]["labels"], res[1]["labels"]]), r["labels"].cpu().numpy())
    for k in (0, 1):
        assert np.max(np.abs(res[k]["centers"] - r["centers"])) <= 1e-12 * np.max(np.abs(r["centers"]))
        assert res[k]["n_iter"] == r["n_iter"]
    assert np.array_equal(res[0]["seeded"], res[1]["seeded"])     # every rank ends with the same centers
    s = vc.kmeans(Xd, C0.shape[0], n_init=2, seed=8)
    assert np.max(np.abs(res[0]["seeded"] - s["centers"])) <= 1e-9 * np.max(np.abs(s["centers"]))
