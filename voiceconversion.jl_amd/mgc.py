"""sp2mc, mc2sp and mc2b of MelGeneralizedCepstrums (third party): the spectral-envelope transforms either side of a
conversion -- call sites test/vc.jl:16,28, bin/vc.jl:71,87, bin/mcep.jl:50, test/diffvc.jl:33, bin/diffvc.jl:83.

A 1-D vector is one frame (a 1-D result comes back).  A (rows, T) host array goes through the host-pointer entry.  A float64
tensor on the HIP device with unit stride along its first axis goes through the `_dev` entry on the current stream and the
result is a new device tensor, so sp2mc -> fvconvert -> mc2sp chains in HBM.  The `_dev` entries do not check the values:
a non-positive power there gives NaN or -inf instead of an error."""
import numpy as np

from . import _lib
from ._arrays import current_stream_ptr, dev_matrix, is_torch, jl_matrix


def _is_device(x):
    return is_torch(x) and x.is_cuda


def _host(x, name):
    """(matrix, was_vector) of a host argument (numpy, list or CPU tensor)."""
    a = np.asarray(x.detach().numpy() if is_torch(x) else x, dtype=np.float64)
    if a.ndim == 1:
        return np.asfortranarray(a.reshape(-1, 1)), True
    return jl_matrix(a, name), False


def _dev_out(rows, T, like):
    import torch

    return torch.empty((T, rows), dtype=torch.float64, device=like.device).t()   # (rows, T), unit stride along rows


def _dev_in(x, name):
    """(tensor as a matrix, was_vector) of a device argument."""
    if x.dim() == 1:
        return x.reshape(-1, 1), True
    return x, False


def sp2mc(sp, order, alpha):
    """sp2mc(sp (K,T), order, alpha) -> (order+1, T): mel-cepstrum of a power spectral envelope (K = fftlen/2 + 1)."""
    order, alpha = int(order), float(alpha)
    if _is_device(sp):
        x, vec = _dev_in(sp, "sp")
        ptr, K, T, ld = dev_matrix(x, "sp")
        out = _dev_out(order + 1, T, x)
        if T == 0:                                    # an empty tensor has no data pointer
            return out
        _lib.check(_lib.lib.vcmi_sp2mc_dev(ptr, ld, K, T, order, alpha, out.data_ptr(), order + 1, current_stream_ptr()))
        return out[:, 0] if vec else out
    x, vec = _host(sp, "sp")
    K, T = x.shape
    out = np.empty((order + 1, T), order="F")
    _lib.check(_lib.lib.vcmi_sp2mc(_lib.dptr(x), K, T, order, alpha, _lib.dptr(out)))
    return out[:, 0] if vec else out


def mc2sp(mc, alpha, fftlen):
    """mc2sp(mc (D,T), alpha, fftlen) -> (fftlen//2 + 1, T): power spectral envelope of a mel-cepstrum; fftlen may be odd
    (the reference passes 2 size(sp, 1) - 1)."""
    alpha, fftlen = float(alpha), int(fftlen)
    K = max(fftlen // 2 + 1, 0)                       # (a bad fftlen is reported by the library)
    if _is_device(mc):
        x, vec = _dev_in(mc, "mc")
        ptr, D, T, ld = dev_matrix(x, "mc")
        out = _dev_out(K, T, x)
        if T == 0:                                    # an empty tensor has no data pointer
            return out
        _lib.check(_lib.lib.vcmi_mc2sp_dev(ptr, ld, D, T, alpha, fftlen, out.data_ptr(), K, current_stream_ptr()))
        return out[:, 0] if vec else out
    x, vec = _host(mc, "mc")
    D, T = x.shape
    out = np.empty((K, T), order="F")
    _lib.check(_lib.lib.vcmi_mc2sp(_lib.dptr(x), D, T, alpha, fftlen, _lib.dptr(out)))
    return out[:, 0] if vec else out


def mc2b(mc, alpha):
    """mc2b(mc (D,T), alpha) -> (D,T): MLSA filter coefficients of a mel-cepstrum."""
    alpha = float(alpha)
    if _is_device(mc):
        x, vec = _dev_in(mc, "mc")
        ptr, D, T, ld = dev_matrix(x, "mc")
        out = _dev_out(D, T, x)
        if T == 0:                                    # an empty tensor has no data pointer
            return out
        _lib.check(_lib.lib.vcmi_mc2b_dev(ptr, ld, D, T, alpha, out.data_ptr(), D, current_stream_ptr()))
        return out[:, 0] if vec else out
    x, vec = _host(mc, "mc")
    D, T = x.shape
    out = np.empty((D, T), order="F")
    _lib.check(_lib.lib.vcmi_mc2b(_lib.dptr(x), D, T, alpha, _lib.dptr(out)))
    return out[:, 0] if vec else out
