"""numpy restatement of sklearn 0.17 cluster.KMeans as the library defines it (test helper, not a test module):
direct-difference distances summed sequentially over dimensions with one rounding per operation, exact ties to the
smaller center index, greedy k-means++ (sklearn _k_init) drawing from numpy default_rng, tolerance scaled by
mean(var(X, axis=0)), empty clusters moved to the frames of largest distance (ties: smaller frame index), best-inertia
centers, one relabelling pass.  Frames are ROWS here: X (N,Dj), centers (M,Dj)."""
import numpy as np


def direct(X, C):
    """(N,M) sum_d (x_d - c_d)^2, sequential in d (the device's order and rounding)."""
    D = np.zeros((X.shape[0], C.shape[0]))
    for d in range(X.shape[1]):
        t = X[:, d, None] - C[None, :, d]
        D = D + t * t
    return D


def assign(X, C):
    D = direct(X, C)
    lab = np.argmin(D, axis=1)                       # first minimum: ties to the smaller index
    return lab, D[np.arange(len(X)), lab]


def update(X, C, lab, d2):
    N, M = len(X), len(C)
    counts = np.bincount(lab, minlength=M)
    newC = C.copy()
    for m in np.nonzero(counts)[0]:
        newC[m] = X[lab == m].sum(axis=0) / counts[m]
    empty = np.nonzero(counts == 0)[0]
    if len(empty):
        order = np.lexsort((np.arange(N), -d2))       # d2 descending, then frame index ascending
        for e, m in enumerate(empty):
            newC[m] = X[order[e]]
    return newC, empty


def lloyd(X, C0, max_iter=300, tol_abs=0.0):
    """-> (centers, inertia, n_iter, labels, history [(labels, centers after update, inertia)])."""
    C = np.array(C0, dtype=np.float64)
    best, best_in, hist = None, None, []
    for it in range(max_iter):
        lab, d2 = assign(X, C)
        inertia = d2.sum()
        newC, _ = update(X, C, lab, d2)
        shift = ((newC - C) ** 2).sum()
        if best_in is None or inertia < best_in:
            best, best_in = newC.copy(), inertia
        hist.append((lab, newC, inertia))
        C = newC
        if shift <= tol_abs:
            break
    lab, d2 = assign(X, best)
    return best, d2.sum(), it + 1, lab, hist


def kpp(X, M, rng):
    """Greedy k-means++ -> (frame indices, smallest distance of a target u*potential to a prefix boundary, relative)."""
    N = len(X)
    L = 2 + int(np.log(M))
    i0 = int(rng.integers(N))
    picks = [i0]
    closest = direct(X, X[i0:i0 + 1])[:, 0]
    pot = closest.sum()
    margin = np.inf
    for _ in range(1, M):
        T = rng.random(L) * pot
        cum = np.cumsum(closest)
        ids = np.minimum(np.searchsorted(cum, T), N - 1)
        for t in T:
            margin = min(margin, np.min(np.abs(cum - t)) / pot)
        dc = direct(X, X[ids])
        pots = np.minimum(closest[:, None], dc).sum(axis=0)
        b = int(np.argmin(pots))
        picks.append(int(ids[b]))
        pot = pots[b]
        closest = np.minimum(closest, dc[:, b])
    return picks, margin


def tolerance(X, tol):
    return float(np.mean(np.var(X, axis=0)) * tol)


def kmeans(X, M, n_init=10, max_iter=300, tol=1e-4, seed=0):
    rng = np.random.default_rng(seed)
    tol_abs = tolerance(X, tol)
    best = None
    for _ in range(n_init):
        picks, _ = kpp(X, M, rng)
        C, inertia, n_iter, lab, _ = lloyd(X, X[picks], max_iter, tol_abs)
        if best is None or inertia < best[1]:
            best = (C, inertia, n_iter, lab)
    return best
