"""GMM training with the EM state resident on the GPU -- what `gmm[:fit](dataset.X')` does in the reference's
bin/train_gmm.jl:84-103 (sklearn.mixture.GMM(n_components, covariance_type="full", n_iter, n_init, min_covar),
optionally refined from a saved model, :92-99).

The hot loop (E-step statistics, M-step, Cholesky whitening of every mixture) never leaves HBM; with a
torch.distributed process group every rank holds a shard of the frames and the only exchange per iteration is ONE
all-reduce of the packed statistics.

Initialisation.  The old sklearn GMM's init_params="wmc" runs KMeans over ALL of X (k-means++ seeding, n_init=10) and
takes np.cov of all of X for every mixture.  Two initialisations are offered:
  * init="subsample" (the default, unchanged): host-side numpy on a random subsample of rank 0's shard -- one plain
    k-means++ seeding and 10 Lloyd iterations, np.cov of the same subsample.  An approximation of sklearn's, cheap
    on the CPU.
  * init="kmeans": sklearn's semantics on the device -- kmeans(X, M) over every frame of every rank (kmeans.py) and
    cov(X) + min_covar I (ddof=1) over every frame, from the M=1 full E-step statistics (N, sum x, sum x x').

covariance_type="diag" runs the same loop on a diagonal model (DiagEMState, vcmi_gmm_em_diag_*): the statistics are the
M(1+2Dj)+1 doubles of the diagonal E-step, the initial variances the diagonal of the data covariance + min_covar (what the
old sklearn GMM takes for "diag") -- for init="kmeans" from the M=1 DIAGONAL E-step statistics (N, sum x, sum x^2), not
the Dj^2 pass.  expand_diag turns its variances into the (Dj,Dj,M) tensor that refine= of the full fit takes.

covariance_type="block_diag" is the cross-diagonal joint model GMM voice conversion is usually trained with (Toda, Black and
Tokuda 2007): Dj is even, D = Dj/2, dimension d couples with dimension d + D only.  BlockDiagEMState (vcmi_gmm_em_bdiag_*)
keeps covars (Dj + D, M) = [variances; cross-covariances c_dm]; the statistics are the M(1 + 2Dj + D) + 1 doubles of the
block-diagonal E-step, the initial covariances the variances and pair covariances of the data + min_covar on the variances --
for init="kmeans" from the M=1 block-diagonal E-step statistics (data_block_covariance).  expand_block_diag gives the
(Dj,Dj,M) tensor that GMMMap and refine= of the full fit take; BlockDiagGMMMap(weights, means, covars) converts frame by
frame with the result as it is (no expansion), TrajectoryGMMMap(precision="diag") converts with such a model exactly.

One driver serves the three types.  train_gmm holds the only EM loop, the only best-of-n_init selection and the only
pack / broadcast / unpack of rank 0's model (pack_model, unpack_model: a third parameter of any shape); what differs between
the types is one _CovType entry of _COV_TYPES -- the state class, the argument check, the covariance entry every mixture
starts from (over all frames, or over a host subsample: subsample_model, numpy only) and the result's "covariance_type".
data_covariance, data_variance and data_block_covariance share _data_moments (unit parameters, the M=1 E-step, the
all-reduce).  Every argument error is raised before the first collective or device call.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._arrays import current_stream_ptr, jl_matrix, jl_vector
from .estep import (_dense_frames, bdiag_stats_len, estep_bdiag_dev, estep_diag_dev, estep_full_dev, full_stats_len, stats_len,
                    unpack_bdiag_stats, unpack_full_stats, unpack_stats)
from .kmeans import kmeans


class _EMState:
    """The handle of a device-resident EM state and the calls of one iteration.  A subclass supplies its C entries (create,
    destroy, estep_dev, mstep, get), the length of its statistics and the shape of its third parameter."""
    _entries = _stats_len = None

    @staticmethod
    def _third_shape(Dj, M):
        raise NotImplementedError

    def _create(self, w, mu, third, name, min_covar):
        w = jl_vector(w)
        mu = jl_matrix(mu, "mu")
        third = np.asfortranarray(np.asarray(third, dtype=np.float64))
        Dj, M = mu.shape
        if third.shape != self._third_shape(Dj, M) or w.shape != (M,):
            raise _lib.DimensionMismatch(f"w {w.shape}, mu {mu.shape}, {name} {third.shape} are inconsistent")
        self.Dj, self.M = Dj, M
        h = C.c_void_p()
        _lib.check(self._entries[0](Dj, M, _lib.dptr(w), _lib.dptr(mu), _lib.dptr(third), float(min_covar), C.byref(h)))
        self._h = h

    def __del__(self):     # (the entries are bound when the subclass is defined: module globals may be gone at exit)
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._entries[1](h)

    def estep(self, X, out=None):
        """Local statistics of the (Dj,N) device block X -> packed device tensor [S0 | S1 | S2 | loglik]."""
        import torch

        ptr, N = _dense_frames(X, self.Dj)
        if out is None:
            out = torch.empty(self._stats_len(self.Dj, self.M), dtype=torch.float64, device=X.device)
        _lib.check(self._entries[2](self._h, ptr, N, out.data_ptr(), current_stream_ptr()))
        return out

    def mstep(self, stats):
        """Parameters <- statistics (already summed over ranks); returns the log-likelihood they carry."""
        ll = np.zeros(1)
        _lib.check(self._entries[3](self._h, stats.data_ptr(), current_stream_ptr(), _lib.dptr(ll)))
        return float(ll[0])

    def get(self):
        w = np.empty(self.M)
        mu = np.empty((self.Dj, self.M), order="F")
        third = np.empty(self._third_shape(self.Dj, self.M), order="F")
        _lib.check(self._entries[4](self._h, _lib.dptr(w), _lib.dptr(mu), _lib.dptr(third)))
        return w, mu, third


class EMState(_EMState):
    """Device-resident (w, mu, Sigma) + whitening blocks of a full-covariance GMM (vcmi_gmm_em_*)."""
    _entries = (_lib.lib.vcmi_gmm_em_create, _lib.lib.vcmi_gmm_em_destroy, _lib.lib.vcmi_gmm_em_estep_dev,
                _lib.lib.vcmi_gmm_em_mstep, _lib.lib.vcmi_gmm_em_get)
    _stats_len = staticmethod(full_stats_len)

    @staticmethod
    def _third_shape(Dj, M):
        return (Dj, Dj, M)

    def __init__(self, w, mu, sigma, min_covar=1e-7):
        self._create(w, mu, sigma, "sigma", min_covar)


class DiagEMState(_EMState):
    """Device-resident (w, mu, var) of a diagonal-covariance GMM (vcmi_gmm_em_diag_*): mu, var are (Dj,M)."""
    _entries = (_lib.lib.vcmi_gmm_em_diag_create, _lib.lib.vcmi_gmm_em_diag_destroy, _lib.lib.vcmi_gmm_em_diag_estep_dev,
                _lib.lib.vcmi_gmm_em_diag_mstep, _lib.lib.vcmi_gmm_em_diag_get)
    _stats_len = staticmethod(stats_len)

    @staticmethod
    def _third_shape(Dj, M):
        return (Dj, M)

    def __init__(self, w, mu, var, min_covar=1e-7):
        self._create(w, mu, var, "var", min_covar)


class BlockDiagEMState(_EMState):
    """Device-resident (w, mu, covars) of a cross-diagonal GMM (vcmi_gmm_em_bdiag_*): mu (Dj,M), covars (Dj + Dj/2, M) =
    [variances; cross-covariances of the pairs (d, d + Dj/2)]."""
    _entries = (_lib.lib.vcmi_gmm_em_bdiag_create, _lib.lib.vcmi_gmm_em_bdiag_destroy, _lib.lib.vcmi_gmm_em_bdiag_estep_dev,
                _lib.lib.vcmi_gmm_em_bdiag_mstep, _lib.lib.vcmi_gmm_em_bdiag_get)
    _stats_len = staticmethod(bdiag_stats_len)

    @staticmethod
    def _third_shape(Dj, M):
        return (Dj + Dj // 2, M)

    def __init__(self, w, mu, covars, min_covar=1e-7):
        if np.ndim(mu) == 2 and np.shape(mu)[0] % 2:
            raise _lib.DimensionMismatch(f"block_diag: the joint dimension must be even, got {np.shape(mu)[0]}")
        self._create(w, mu, covars, "block_diag covars", min_covar)


def expand_block_diag(covars):
    """covars (Dj + D, M) of a cross-diagonal model -> the (Dj,Dj,M) covariance tensor: the variances on the diagonals, c at
    (d, d + D) and (d + D, d).  What GMMMap and train_gmm(X, refine=(w, mu, expand_block_diag(covars))) take; the native
    frame-by-frame converter of such a model, BlockDiagGMMMap, takes covars itself."""
    v = np.asarray(covars, dtype=np.float64)
    if v.ndim != 2 or v.shape[0] % 3:
        raise _lib.DimensionMismatch(f"expand_block_diag: covars must be (Dj + Dj/2, M), got {v.shape}")
    D, M = v.shape[0] // 3, v.shape[1]
    Dj = 2 * D
    out = np.zeros((Dj, Dj, M), order="F")
    i, d = np.arange(Dj), np.arange(D)
    out[i, i, :] = v[:Dj]
    out[d, d + D, :] = v[Dj:]
    out[d + D, d, :] = v[Dj:]
    return out


def expand_diag(covars):
    """Variances (Dj,M) -> the (Dj,Dj,M) covariance tensor with them on the diagonals:
    train_gmm(X, refine=(w, mu, expand_diag(var))) warm-starts the full-covariance fit from a diagonal one."""
    v = np.asarray(covars, dtype=np.float64)
    if v.ndim != 2:
        raise _lib.DimensionMismatch(f"expand_diag: covars must be (Dj,M), got {v.shape}")
    Dj, M = v.shape
    out = np.zeros((Dj, Dj, M), order="F")
    i = np.arange(Dj)
    out[i, i, :] = v
    return out


def kmeans_init(Xs, M, rng, n_iter=10):
    """k-means++ seeding and a few Lloyd iterations on a host subsample Xs (n,Dj): means for init_params='wmc'."""
    n = Xs.shape[0]
    centers = [Xs[rng.integers(n)]]
    d2 = np.sum((Xs - centers[0]) ** 2, axis=1)
    for _ in range(1, M):
        p = d2 / d2.sum() if d2.sum() > 0 else np.full(n, 1.0 / n)
        centers.append(Xs[rng.choice(n, p=p)])
        d2 = np.minimum(d2, np.sum((Xs - centers[-1]) ** 2, axis=1))
    Cn = np.asarray(centers)
    for _ in range(n_iter):
        dist = (Xs * Xs).sum(1)[:, None] - 2.0 * Xs @ Cn.T + (Cn * Cn).sum(1)[None, :]
        lab = dist.argmin(1)
        for m in range(M):
            sel = lab == m
            if sel.any():
                Cn[m] = Xs[sel].mean(0)
    return Cn


def _data_moments(X, estep, unit, unpack, group):
    """The moments of every frame of every rank: the M=1 E-step of `estep` under unit parameters (weight 1, mean 0, covariance
    entry `unit`), all-reduced -> n, sum x (Dj,) and the type's remaining statistics, each without its mixture axis."""
    import torch.distributed as dist

    Dj = X.shape[0]
    st = estep(X, np.ones(1), np.zeros((Dj, 1)), unit)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(st, group=group)
    S0, S1, *rest = unpack(st.cpu().numpy(), Dj, 1)[:-1]
    return S0[0], S1[:, 0], [S[..., 0] for S in rest]


def data_covariance(X, group=None):
    """cov(X) (ddof=1, as np.cov) over every frame of every rank, from the M=1 full E-step statistics."""
    n, s1, (S2,) = _data_moments(X, estep_full_dev, np.eye(X.shape[0])[:, :, None], unpack_full_stats, group)
    cv = (S2 - np.outer(s1, s1) / n) / (n - 1.0)
    return 0.5 * (cv + cv.T)


def data_variance(X, group=None):
    """var(X) per dimension (ddof=1, the diagonal of np.cov) over every frame of every rank, from the M=1 diagonal E-step
    statistics (N, sum x, sum x^2)."""
    n, s1, (S2,) = _data_moments(X, estep_diag_dev, np.ones((X.shape[0], 1)), unpack_stats, group)
    return (S2 - s1 * s1 / n) / (n - 1.0)


def data_block_covariance(X, group=None):
    """The (Dj + D,) variances and pair covariances cov(z_d, z_{d+D}) (ddof=1) over every frame of every rank, from the M=1
    block-diagonal E-step statistics (N, sum z, sum z^2, sum z_d z_{d+D})."""
    Dj = X.shape[0]
    D = Dj // 2
    n, s1, (S2, Sxy) = _data_moments(X, estep_bdiag_dev, np.vstack([np.ones((Dj, 1)), np.zeros((D, 1))]), unpack_bdiag_stats, group)
    return np.concatenate([S2 - s1 * s1 / n, Sxy - s1[:D] * s1[D:] / n]) / (n - 1.0)


# What train_gmm knows of a covariance type.  state: its _EMState subclass (which has the shape of the third parameter and the
# length of the statistics); check(Dj, M, refine): the argument errors of the type, None where the state's own checks are all
# there are; data_entry(X, group, min_covar) and sample_entry(Xs, min_covar): the covariance entry every mixture starts from,
# over every frame of every rank (init="kmeans") and over a host subsample Xs (n,Dj); label: the result's "covariance_type",
# None for none.
_CovType = namedtuple("_CovType", "state check data_entry sample_entry label")


def _check_diag(Dj, M, refine):
    if refine is not None and np.shape(refine[2]) != (Dj, M):
        raise _lib.DimensionMismatch(f"train_gmm: covariance_type='diag' refines from variances ({Dj},{M}), got {np.shape(refine[2])}")


def _check_block_diag(Dj, M, refine):
    if Dj % 2:
        raise _lib.DimensionMismatch(f"train_gmm: covariance_type='block_diag' needs an even joint dimension, got {Dj}")
    if refine is not None and np.shape(refine[2]) != (Dj + Dj // 2, M):
        raise _lib.DimensionMismatch(f"train_gmm: covariance_type='block_diag' refines from covars ({Dj + Dj // 2},{M}), got {np.shape(refine[2])}")


def _block_diag_floor(Dj, min_covar):
    """min_covar on the variances only"""
    return np.concatenate([np.full(Dj, float(min_covar)), np.zeros(Dj // 2)])


def _block_diag_sample_entry(Xs, min_covar):
    Dj = Xs.shape[1]
    D = Dj // 2
    Xc = Xs - Xs.mean(axis=0)
    pair = (Xc[:, :D] * Xc[:, D:]).sum(axis=0) / (len(Xs) - 1.0)
    return np.concatenate([np.var(Xs, axis=0, ddof=1), pair]) + _block_diag_floor(Dj, min_covar)


_COV_TYPES = {
    "full": _CovType(EMState, None,
                     lambda X, group, min_covar: data_covariance(X, group) + min_covar * np.eye(X.shape[0]),
                     lambda Xs, min_covar: np.cov(Xs.T) + min_covar * np.eye(Xs.shape[1]), None),
    "diag": _CovType(DiagEMState, _check_diag,
                     lambda X, group, min_covar: data_variance(X, group) + min_covar,
                     lambda Xs, min_covar: np.var(Xs, axis=0, ddof=1) + min_covar, "diag"),
    "block_diag": _CovType(BlockDiagEMState, _check_block_diag,
                           lambda X, group, min_covar: data_block_covariance(X, group) + _block_diag_floor(X.shape[0], min_covar),
                           _block_diag_sample_entry, "block_diag"),
}


def subsample_model(Xs, M, rng, min_covar, covariance_type):
    """The initial model of init="subsample" from the host subsample Xs (n,Dj), numpy only: uniform weights, the means of
    kmeans_init (the only draws from rng) and the type's covariance entry of Xs for every mixture -> w (M,), mu (Dj,M) and
    the third parameter in its Julia shape (...,M)."""
    mu0 = kmeans_init(Xs, M, rng).T
    entry = _COV_TYPES[covariance_type].sample_entry(Xs, min_covar)
    return np.full(M, 1.0 / M), mu0, np.repeat(entry[..., None], M, axis=-1)


def pack_model(w, mu, third):
    """w (M,), mu (Dj,M) and a third parameter of any shape -> one vector, every array in Julia (column-major) order: what rank 0
    broadcasts"""
    return np.concatenate([np.ravel(np.asarray(a, dtype=np.float64), order="F") for a in (w, mu, third)])


def unpack_model(h, Dj, M, third_shape):
    """the inverse of pack_model"""
    return h[:M].copy(), h[M:M + M * Dj].reshape((Dj, M), order="F"), h[M + M * Dj:].reshape(third_shape, order="F")


def train_gmm(X, n_components=16, n_iter=200, n_init=2, min_covar=1e-7, tol=1e-3, refine=None, seed=0, group=None,
              init_sample=50000, init="subsample", covariance_type="full"):
    """train_gmm.jl's `gmm[:fit]`: X is this rank's (Dj,N) device-resident shard of the joint features.

    n_init random initialisations (k-means means, uniform weights, the data covariance + min_covar*I for every
    mixture -- the old sklearn GMM's init_params='wmc'), each run for at most n_iter EM iterations or until the mean
    log-likelihood per frame changes by less than tol; the best final log-likelihood wins.  refine=(w, mu, Sigma)
    starts from a pretrained model instead (bin/train_gmm.jl:92-99, init_params='').  init="kmeans" takes the means from
    kmeans over every frame of every rank and the covariance of every frame (see the module docstring); the default
    "subsample" keeps the host-side subsample initialisation.
    Returns {"weights", "means" (Dj,M), "covars" (Dj,Dj,M), "n_components", "loglik" (per-frame history), "converged"}.
    covariance_type="diag" fits a diagonal model by the same rules (module docstring): refine=(w, mu, var (Dj,M)), the
    variances start from the diagonal of the data covariance + min_covar, "covars" is (Dj,M) and the result carries
    "covariance_type": "diag".
    covariance_type="block_diag" fits the cross-diagonal model (module docstring; Dj even): refine=(w, mu, covars (Dj + Dj/2, M)),
    "covars" is (Dj + Dj/2, M) = [variances; pair cross-covariances] and the result carries "covariance_type": "block_diag".
    Argument errors are raised before the first collective or device call.
    """
    if covariance_type not in tuple(_COV_TYPES):
        raise ValueError(f"train_gmm: covariance_type must be 'full', 'diag' or 'block_diag', got {covariance_type!r}")
    ct = _COV_TYPES[covariance_type]
    Dj, N = X.shape
    M = int(n_components)
    if ct.check is not None:
        ct.check(Dj, M, refine)
    if init not in ("subsample", "kmeans"):
        raise ValueError(f"train_gmm: init must be 'subsample' or 'kmeans', got {init!r}")

    import torch
    import torch.distributed as dist

    distributed = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank(group) if distributed else 0
    ntot = torch.tensor([float(N)], dtype=torch.float64, device=X.device)
    if distributed:
        dist.all_reduce(ntot, group=group)
    ntot = float(ntot.item())
    rng = np.random.default_rng(seed)
    third_shape = ct.state._third_shape(Dj, M)
    entry_all = ct.data_entry(X, group, min_covar) if init == "kmeans" and refine is None else None
    best = None
    for _ in range(1 if refine is not None else max(1, int(n_init))):
        if refine is not None:
            w0, mu0, third0 = refine
        elif init == "kmeans":
            # every rank runs the same collective k-means and gets the same centers: nothing to broadcast
            mu0 = kmeans(X, M, seed=int(rng.integers(2**31 - 1)), group=group)["centers"]
            third0 = np.repeat(entry_all[..., None], M, axis=-1)
            w0 = np.full(M, 1.0 / M)
        else:
            # rank 0 draws the initial model from its shard and every rank receives the same one
            pk = torch.empty(M * (1 + Dj) + int(np.prod(third_shape)), dtype=torch.float64, device=X.device)
            if rank == 0:
                idx = rng.choice(N, size=min(N, int(init_sample)), replace=False)
                Xs = X[:, torch.from_numpy(np.sort(idx)).to(X.device)].t().contiguous().cpu().numpy()
                pk.copy_(torch.from_numpy(pack_model(*subsample_model(Xs, M, rng, min_covar, covariance_type))))
            if distributed:
                dist.broadcast(pk, src=0, group=group)
            w0, mu0, third0 = unpack_model(pk.cpu().numpy(), Dj, M, third_shape)
        em = ct.state(w0, mu0, third0, min_covar)
        stats = torch.empty(em._stats_len(Dj, M), dtype=torch.float64, device=X.device)
        hist, converged = [], False
        for _ in range(int(n_iter)):
            em.estep(X, out=stats)
            if distributed:
                dist.all_reduce(stats, group=group)
            hist.append(em.mstep(stats) / ntot)
            if len(hist) > 1 and abs(hist[-1] - hist[-2]) < tol:
                converged = True
                break
        if best is None or hist[-1] > best[0]:
            best = (hist[-1], em.get(), hist, converged)
    (w, mu, covars), hist, converged = best[1], best[2], best[3]
    out = {"weights": w, "means": mu, "covars": covars, "n_components": M, "loglik": hist, "converged": converged}
    if ct.label is not None:
        out["covariance_type"] = ct.label
    return out


__all__ = ["EMState", "DiagEMState", "BlockDiagEMState", "train_gmm", "expand_diag", "expand_block_diag", "data_block_covariance", "kmeans_init", "data_covariance", "data_variance", "unpack_full_stats"]
