"""BlockDiagGMMMap: frame-by-frame conversion (src/gmmmap.jl:1-118) with a CROSS-DIAGONAL joint GMM -- the model that
train_gmm(covariance_type="block_diag") returns, converted as it is: no (Dj,Dj,M) tensor, no Cholesky, no dense kernel."""
import ctypes as C

import numpy as np

from . import _lib
from ._arrays import current_stream_ptr, dev_matrix, is_torch, jl_matrix, jl_vector, sigma2_arg
from .common import FrameByFrameConverter
from .gmm import GMM


class BlockDiagGMMMap(FrameByFrameConverter):
    """BlockDiagGMMMap(weights (M,), mu (Dj,M), covars (Dj + Dj/2, M); swap=False): covars = [variances of the Dj rows; Dj/2 pair
    cross-covariances], pair d = rows (d, d + Dj/2).  Equal to GMMMap(weights, mu, expand_block_diag(covars), swap) to rounding
    (include/vcmi.h: vcmi_bdmap_*; csrc/gmmmap_bdiag.hip).  Converts on the device it was created on."""

    def __init__(self, weights, mu, covars, swap=False):
        w = jl_vector(weights)
        mu = jl_matrix(mu, "μ")
        cov = jl_matrix(covars, "covars")
        Dj, M = mu.shape
        if Dj < 2 or Dj % 2:
            raise _lib.DimensionMismatch(f"the joint dimension must be even and at least 2, got {Dj}")
        if w.shape != (M,) or cov.shape != (Dj + Dj // 2, M):
            raise _lib.DimensionMismatch(f"weights {w.shape}, μ {mu.shape}, covars {cov.shape} are inconsistent: "
                                         f"covars must be (Dj + Dj/2, M) = ({Dj + Dj // 2}, {M})")
        if Dj // 2 > 128 or M > 256:
            raise _lib.DimensionMismatch(f"dimension {Dj // 2} / {M} mixtures exceed the cross-diagonal converter's limits (128, 256)")
        h = C.c_void_p()
        _lib.check(_lib.lib.vcmi_bdmap_create(_lib.dptr(w), _lib.dptr(mu), _lib.dptr(cov), Dj, M, int(bool(swap)), C.byref(h)))
        self._h = h
        self._D, self._M = Dj >> 1, M
        self.px = GMM(self, "vcmi_bdmap")

    def __del__(self, _destroy=_lib.lib.vcmi_bdmap_destroy):     # bound at definition: module globals may be gone at exit
        h = getattr(self, "_h", None)
        if h:
            _destroy(h)
            self._h = None

    def __len__(self):
        return 1

    def _dim(self):
        return _lib.lib.vcmi_bdmap_dim(self._h)

    def _ncomponents(self):
        return _lib.lib.vcmi_bdmap_ncomponents(self._h)

    @property
    def slopes(self):
        """a = c / vˣ (D,M): the diagonal of GMMMap's ΣʸˣΣˣˣ⁻¹"""
        a = np.empty((self._D, self._M), order="F")
        _lib.check(_lib.lib.vcmi_bdmap_get_a(self._h, _lib.dptr(a)))
        return a

    def _fvconvert(self, x, out=None):
        if is_torch(x):
            import torch

            ptr, D, T, ld = dev_matrix(x, "X")
            if D != self._D:
                raise _lib.DimensionMismatch("Inconsistent dimentions.")
            if out is None:
                out = torch.empty((T, D), dtype=torch.float64, device=x.device).t()
            optr, oD, oT, old = dev_matrix(out, "out")
            if (oD, oT) != (D, T):
                raise _lib.DimensionMismatch("output shape does not match input")
            _lib.check(_lib.lib.vcmi_bdmap_convert_dev(self._h, ptr, ld, T, optr, old, current_stream_ptr()))
            return out
        x = np.asarray(x)
        if x.ndim == 1:
            v = jl_vector(x)
            if len(v) != self._D:
                raise _lib.DimensionMismatch("Inconsistent dimentions.")
            y = np.empty(self._D)
            _lib.check(_lib.lib.vcmi_bdmap_convert(self._h, _lib.dptr(v), self._D, 1, _lib.dptr(y), self._D))
            return y
        X = jl_matrix(x, "X")
        D, T = X.shape
        if D != self._D:
            raise _lib.DimensionMismatch("Inconsistent dimentions.")
        if out is None:
            Y = np.empty((D, T), order="F")
        else:
            Y = out
            if Y.shape != (D, T) or Y.dtype != np.float64 or not Y.flags.f_contiguous:
                raise _lib.DimensionMismatch("out must be a Fortran-ordered float64 (D,T) array")
        _lib.check(_lib.lib.vcmi_bdmap_convert(self._h, _lib.dptr(X), D, T, _lib.dptr(Y), D))
        return Y

    def _vc(self, fm, postfilter=None):          # src/common.jl:7-26 (+ fvpostf! of src/gv.jl:10-15 before the download)
        fm = jl_matrix(fm, "fm")
        if fm.shape[0] != self._D + 1:
            raise _lib.DimensionMismatch("Inconsistent dimentions.")
        s2 = sigma2_arg(postfilter, self._D)
        out = np.empty_like(fm, order="F")
        _lib.check(_lib.lib.vcmi_vc_bdmap(self._h, _lib.dptr(fm), fm.shape[1], s2, _lib.dptr(out)))
        return out

    def _vc_batch(self, fms, postfilter=None):
        fms = [jl_matrix(f, "fm") for f in fms]
        n = len(fms)
        if n == 0:
            return []
        for f in fms:
            if f.shape[0] != self._D + 1:
                raise _lib.DimensionMismatch("Inconsistent dimentions.")
        s2 = sigma2_arg(postfilter, self._D)
        T = np.array([f.shape[1] for f in fms], dtype=np.int64)
        outs = [np.empty_like(f, order="F") for f in fms]
        dpp = C.POINTER(C.c_double) * n
        _lib.check(_lib.lib.vcmi_vc_bdmap_batch(self._h, n, dpp(*[_lib.dptr(f) for f in fms]), _lib.iptr(T), s2,
                                                dpp(*[_lib.dptr(o) for o in outs])))
        return outs
