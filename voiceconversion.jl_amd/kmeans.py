"""k-means over every frame on the device -- sklearn 0.17 cluster.KMeans, which the reference's
sklearn.mixture.GMM(init_params="wmc") runs over all of X for each of its n_init initialisations (bin/train_gmm.jl:84-89).

kmeans(X, n_clusters, n_init=10, max_iter=300, tol=1e-4, seed=0, init=None, group=None) takes this rank's (Dj,N)
device shard.  Semantics: greedy k-means++ seeding (2 + floor(ln M) local trials), Lloyd iterations until the summed
squared shift of the centers is <= tol * mean(var(X)), empty clusters moved to the frames farthest from their centers,
best inertia over n_init runs, one relabelling pass after the last update.  Every distance is the direct difference
sum_d (x_d - c_d)^2; exact ties go to the smaller center index.  Random numbers are drawn on the host
(numpy default_rng(seed)), never on the device.

With a torch.distributed process group every rank keeps its frames; per Lloyd iteration the only exchange is one
all-reduce of the packed statistics [count (M) | sum x (Dj,M) | inertia].  Every collective here is an all-reduce(sum)
(a gather is an all-reduce of a zero buffer with the rank's own slot filled: adding zeros is exact)."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._arrays import current_stream_ptr, dev_matrix, jl_matrix


def kmeans_stats_len(Dj, M):
    return int(_lib.lib.vcmi_kmeans_stats_len(int(Dj), int(M)))


class KMeansState:
    """Device-resident centers (Dj,M) of one k-means run and the per-frame state of the last pass (vcmi_kmeans_*)."""

    def __init__(self, Dj, M, centers=None):
        self.Dj, self.M = int(Dj), int(M)
        c = None
        if centers is not None:
            c = jl_matrix(centers, "centers")
            if c.shape != (self.Dj, self.M):
                raise _lib.DimensionMismatch(f"centers {c.shape} is not ({self.Dj},{self.M})")
        h = C.c_void_p()
        _lib.check(_lib.lib.vcmi_kmeans_create(self.Dj, self.M, _lib.dptr(c) if c is not None else None, C.byref(h)))
        self._h = h

    def __del__(self, _destroy=_lib.lib.vcmi_kmeans_destroy):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _destroy(h)

    def _x(self, X):
        ptr, D, N, ld = dev_matrix(X, "X")
        if D != self.Dj or (N > 1 and ld != self.Dj):
            raise _lib.DimensionMismatch("X must be a dense (Dj,N) device matrix matching the centers' dimension")
        return ptr, N

    def assign(self, X, labels=None, out=None):
        """Local statistics of X -> packed device tensor [count (M) | sum x (Dj,M) | inertia]; labels (int32, N) optional."""
        import torch

        ptr, N = self._x(X)
        if out is None:
            out = torch.empty(kmeans_stats_len(self.Dj, self.M), dtype=torch.float64, device=X.device)
        lp = None
        if labels is not None:
            if labels.dtype != torch.int32 or labels.numel() != N or not labels.is_contiguous():
                raise ValueError("labels must be a contiguous int32 device tensor of N entries")
            lp = labels.data_ptr()
        _lib.check(_lib.lib.vcmi_kmeans_assign_dev(self._h, ptr, N, out.data_ptr(), lp, current_stream_ptr()))
        return out

    def update(self, stats):
        """centers <- sum x / count; returns (shift (NaN while empty clusters wait for relocate), inertia, n_empty)."""
        shift, inertia, ne = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
        _lib.check(_lib.lib.vcmi_kmeans_update(self._h, stats.data_ptr(), current_stream_ptr(), C.byref(shift), C.byref(inertia),
                                               C.byref(ne)))
        return shift.value, inertia.value, ne.value

    def far(self, X, E, offset=0):
        """This block's top-E records [mind2, global index, x (Dj)] of the last assignment -> (E, Dj+2) device tensor."""
        import torch

        ptr, N = self._x(X)
        rec = torch.empty((int(E), self.Dj + 2), dtype=torch.float64, device=X.device)
        _lib.check(_lib.lib.vcmi_kmeans_far_dev(self._h, ptr, N, int(E), int(offset), rec.data_ptr(), current_stream_ptr()))
        return rec

    def relocate(self, stats, cand):
        shift = C.c_double(0.0)
        cand = cand.contiguous()
        _lib.check(_lib.lib.vcmi_kmeans_relocate(self._h, stats.data_ptr(), cand.data_ptr(), cand.shape[0], current_stream_ptr(),
                                                 C.byref(shift)))
        return shift.value

    def seed_commit(self, X, c, center):
        ptr, N = self._x(X)
        center = center.contiguous()
        pot = C.c_double(0.0)
        _lib.check(_lib.lib.vcmi_kmeans_seed_commit(self._h, ptr, N, int(c), center.data_ptr(), current_stream_ptr(), C.byref(pot)))
        return pot.value

    def seed_pick(self, targets):
        t = np.ascontiguousarray(targets, dtype=np.float64)
        idx = np.zeros(len(t), dtype=np.int64)
        _lib.check(_lib.lib.vcmi_kmeans_seed_pick(self._h, len(t), _lib.dptr(t), current_stream_ptr(), _lib.iptr(idx)))
        return idx

    def seed_trials(self, X, cand):
        """cand: (L, Dj) contiguous device tensor (L candidate centers) -> local potentials (L,)."""
        ptr, N = self._x(X)
        cand = cand.contiguous()
        pots = np.zeros(cand.shape[0])
        _lib.check(_lib.lib.vcmi_kmeans_seed_trials(self._h, ptr, N, cand.data_ptr(), cand.shape[0], current_stream_ptr(),
                                                    _lib.dptr(pots)))
        return pots

    def mind2(self, N, device):
        """Direct-difference squared distance of each of the last pass's N frames to its nearest center (device tensor)."""
        import torch

        out = torch.empty(int(N), dtype=torch.float64, device=device)
        _lib.check(_lib.lib.vcmi_kmeans_mind2_dev(self._h, int(N), out.data_ptr(), current_stream_ptr()))
        return out

    def set(self, centers):
        c = jl_matrix(centers, "centers")
        if c.shape != (self.Dj, self.M):
            raise _lib.DimensionMismatch(f"centers {c.shape} is not ({self.Dj},{self.M})")
        _lib.check(_lib.lib.vcmi_kmeans_set(self._h, _lib.dptr(c)))

    def get(self):
        c = np.empty((self.Dj, self.M), order="F")
        _lib.check(_lib.lib.vcmi_kmeans_get(self._h, _lib.dptr(c)))
        return c

    def restore_best(self):
        _lib.check(_lib.lib.vcmi_kmeans_restore_best(self._h))


class _Comm:
    """All-reduce(sum) over the group when torch.distributed is initialised; identity otherwise."""

    def __init__(self, group):
        import torch.distributed as dist

        self.on = dist.is_available() and dist.is_initialized()
        self.group = group
        self.rank = dist.get_rank(group) if self.on else 0
        self.world = dist.get_world_size(group) if self.on else 1

    def sum_(self, t):
        if self.on:
            import torch.distributed as dist

            dist.all_reduce(t, group=self.group)
        return t

    def gather_scalar(self, v, device):
        import torch

        t = torch.zeros(self.world, dtype=torch.float64, device=device)
        t[self.rank] = float(v)
        return self.sum_(t).cpu().numpy()


def _mean_variance(X, comm):
    """mean over dimensions of var(X, axis=frames) over all frames of all ranks (sklearn's _tolerance), two passes."""
    Dj = X.shape[0]
    km = KMeansState(Dj, 1, np.zeros((Dj, 1)))
    st = comm.sum_(km.assign(X)).cpu().numpy()
    n = st[0]
    km.set((st[1:1 + Dj] / n).reshape(Dj, 1))
    st = comm.sum_(km.assign(X)).cpu().numpy()
    return st[-1] / (n * Dj)


def _seed(km, X, M, rng, comm, offset, ntot):
    """Greedy k-means++ (sklearn 0.17 _k_init) over the frames of every rank."""
    import torch

    Dj, N = X.shape
    dev = X.device
    L = 2 + int(math.log(M))

    def frames(gidx):
        """(len(gidx), Dj) device tensor of global frames: each owner fills its rows, one all-reduce."""
        out = torch.zeros((len(gidx), Dj), dtype=torch.float64, device=dev)
        for r, g in enumerate(gidx):
            if offset <= g < offset + N:
                out[r] = X[:, g - offset]
        return comm.sum_(out)

    c0 = frames([int(rng.integers(ntot))])[0]
    pots = comm.gather_scalar(km.seed_commit(X, 0, c0), dev)
    current = float(sum(pots))
    for c in range(1, M):
        T = rng.random(L) * current
        before = np.concatenate([[0.0], np.cumsum(pots)[:-1]])
        owners = []
        for t in T:
            r = next((r for r in range(comm.world) if t <= before[r] + pots[r]), None)
            if r is None:
                r = max(r for r in range(comm.world) if pots[r] > 0 or r == 0)
            owners.append(r)
        owners = np.asarray(owners)
        gidx = np.zeros(L)
        mine = owners == comm.rank
        if mine.any():
            gidx[mine] = km.seed_pick(T[mine] - before[comm.rank]) + offset
        gidx = comm.sum_(torch.from_numpy(gidx).to(dev)).cpu().numpy().astype(np.int64)
        cand = frames(gidx)
        tp = torch.from_numpy(km.seed_trials(X, cand)).to(dev)
        tp = comm.sum_(tp).cpu().numpy()
        best = 0
        for l in range(1, L):
            if tp[l] < tp[best]:
                best = l
        pots = comm.gather_scalar(km.seed_commit(X, c, cand[best]), dev)
        current = float(tp[best])
    return km


def _lloyd(km, X, max_iter, tol, comm, offset):
    import torch

    Dj, N = X.shape
    stats = torch.empty(kmeans_stats_len(km.Dj, km.M), dtype=torch.float64, device=X.device)
    for it in range(int(max_iter)):
        comm.sum_(km.assign(X, out=stats))
        shift, inertia, ne = km.update(stats)
        if ne > 0:
            rec = km.far(X, ne, offset)
            if comm.on:
                allrec = torch.zeros((comm.world, ne, km.Dj + 2), dtype=torch.float64, device=X.device)
                allrec[comm.rank] = rec
                rec = comm.sum_(allrec).reshape(comm.world * ne, km.Dj + 2)
            shift = km.relocate(stats, rec)
        if shift <= tol:
            break
    km.restore_best()
    labels = torch.empty(N, dtype=torch.int32, device=X.device)
    comm.sum_(km.assign(X, labels=labels, out=stats))
    return km.get(), float(stats[-1].item()), it + 1, labels


def kmeans(X, n_clusters, n_init=10, max_iter=300, tol=1e-4, seed=0, init=None, group=None):
    """sklearn 0.17 KMeans(n_clusters, init="k-means++" or an array, n_init, max_iter, tol).fit over the frames of every
    rank.  X: this rank's dense (Dj,N) float64 device shard.  Returns {"centers" (Dj,M) numpy, "inertia", "n_iter",
    "labels" (N,) int32 device tensor of this rank's frames}."""
    comm = _Comm(group)
    _, Dj, N, ld = dev_matrix(X, "X")
    M = int(n_clusters)
    if Dj < 1 or M < 1:
        raise _lib.DimensionMismatch(f"kmeans: Dj={Dj}, n_clusters={M}")
    if N > 1 and ld != Dj:
        raise _lib.DimensionMismatch("kmeans: X must be dense (leading dimension Dj)")
    if int(max_iter) < 1:
        raise ValueError("kmeans: max_iter must be >= 1")
    counts = comm.gather_scalar(N, X.device).astype(np.int64)
    ntot = int(counts.sum())
    offset = int(counts[:comm.rank].sum())
    if M > ntot:
        raise _lib.DimensionMismatch(f"kmeans: n_clusters={M} > n_samples={ntot}")
    tol_abs = float(tol) * _mean_variance(X, comm) if tol > 0 else 0.0
    rng = np.random.default_rng(seed)
    best = None
    for _ in range(1 if init is not None else max(1, int(n_init))):
        km = KMeansState(Dj, M, init)
        if init is None:
            _seed(km, X, M, rng, comm, offset, ntot)
        centers, inertia, n_iter, labels = _lloyd(km, X, max_iter, tol_abs, comm, offset)
        if best is None or inertia < best["inertia"]:
            best = {"centers": centers, "inertia": inertia, "n_iter": n_iter, "labels": labels}
    return best


__all__ = ["KMeansState", "kmeans", "kmeans_stats_len"]
