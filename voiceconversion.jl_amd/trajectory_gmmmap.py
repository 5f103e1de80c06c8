"""Trajectory-based (MLPG) conversion -- reference src/trajectory_gmmmap.jl:1-110, push_delta src/datasets.jl:6-13."""
import ctypes as C

import numpy as np

from . import _lib
from ._arrays import current_stream_ptr, dev_matrix, is_torch, jl_matrix, sigma2_arg
from .common import TrajectoryConverter
from .gmmmap_bdiag import BlockDiagGMMMap


def constructW(D, T, windows=2):
    """constructW(D, T): the (2DT x DT) sparse window matrix of src/trajectory_gmmmap.jl:39-61 -- identity for the
    static rows, -1/2 / +1/2 on the neighbouring frames for the delta rows (missing neighbours dropped).
    Host-side helper for API parity (test/trajectory_gmmmap.jl:1-34); the GPU solver applies W as a stencil and
    never materialises it.  windows=3: (3DT x DT), rows [static; delta; delta-delta] per frame, the delta-delta rows 1 / -2 / 1
    on frames t-1, t, t+1 (missing neighbours dropped, the -2 always there): W of BlockDiagTrajectoryGMMMap(g, T, windows=3)."""
    import scipy.sparse as sp

    if windows == 3:
        return _constructW3(D, T)
    if windows != 2:
        raise ValueError("constructW: windows must be 2 (static + delta) or 3 (static + delta + delta-delta)")
    t = np.arange(T)
    d = np.arange(D)
    rows = [(2 * D * t[:, None] + d[None, :]).ravel()]
    cols = [(D * t[:, None] + d[None, :]).ravel()]
    vals = [np.ones(D * T)]
    if T >= 2:
        tt = t[1:]
        rows.append((2 * D * tt[:, None] + D + d[None, :]).ravel())
        cols.append((D * (tt[:, None] - 1) + d[None, :]).ravel())
        vals.append(np.full(D * (T - 1), -0.5))
        tt = t[:-1]
        rows.append((2 * D * tt[:, None] + D + d[None, :]).ravel())
        cols.append((D * (tt[:, None] + 1) + d[None, :]).ravel())
        vals.append(np.full(D * (T - 1), 0.5))
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * D * T, D * T))


def _constructW3(D, T):
    import scipy.sparse as sp

    t = np.arange(T)
    d = np.arange(D)
    rows, cols, vals = [], [], []

    def put(block, tt, shift, v):           # value v in the rows of `block` of frames tt, on the columns of frame tt + shift
        rows.append((3 * D * tt[:, None] + block * D + d[None, :]).ravel())
        cols.append((D * (tt[:, None] + shift) + d[None, :]).ravel())
        vals.append(np.full(D * len(tt), v))

    put(0, t, 0, 1.0)
    put(2, t, 0, -2.0)
    if T >= 2:
        put(1, t[1:], -1, -0.5)
        put(1, t[:-1], 1, 0.5)
        put(2, t[1:], -1, 1.0)
        put(2, t[:-1], 1, 1.0)
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * D * T, D * T))


def push_delta(src, order=1):
    """push_delta(src (D,T)) -> (2D,T), src/datasets.jl:6-13: delta_t = (x_{t+1} - x_{t-1})/2 for 2 <= t <= T-1;
    the first and last frame keep a copy of the static features in the delta rows (repmat artefact).
    A torch tensor on the device gives a device tensor (vcmi_push_delta_dev on the current stream): the trajectory
    converter's input is built where the features are.
    order=2 -> (3D,T): rows 0 .. 2D-1 as above, bit for bit; rows 2D .. 3D-1 the delta-delta x_{t-1} - 2 x_t + x_{t+1} with a
    neighbour outside the matrix dropped (a_1 = -2 x_1 + x_2, a_T = x_{T-1} - 2 x_T) -- the rows of constructW(D, T, windows=3),
    the input of BlockDiagTrajectoryGMMMap(g, T, windows=3) and of its model's training (vcmi_push_delta2[_dev])."""
    if order not in (1, 2):
        raise ValueError("push_delta: order must be 1 (static + delta) or 2 (static + delta + delta-delta)")
    host, dev = ((_lib.lib.vcmi_push_delta, _lib.lib.vcmi_push_delta_dev) if order == 1 else
                 (_lib.lib.vcmi_push_delta2, _lib.lib.vcmi_push_delta2_dev))
    blocks = order + 1
    if is_torch(src):
        import torch

        ptr, D, T, ld = dev_matrix(src, "src")
        buf = torch.empty((T, blocks * D), dtype=torch.float64, device=src.device)
        _lib.check(dev(ptr, ld, D, T, buf.data_ptr(), blocks * D, current_stream_ptr()))
        return buf.t()
    src = jl_matrix(src, "src")
    D, T = src.shape
    out = np.empty((blocks * D, T), order="F")
    _lib.check(host(_lib.dptr(src), D, T, _lib.dptr(out)))
    return out


def _vc_host_args(c, fm, postfilter, delta):
    """fm of vc(c, fm; delta) on the host, (D+1,T) STATIC features if delta else (2D+1,T) -> (fm as a Julia matrix, D, sigma2
    argument)"""
    fm = jl_matrix(fm, "fm")
    D = c._static_dim()
    if fm.shape[0] != (D if delta else c._dim()) + 1:
        raise _lib.DimensionMismatch("Inconsistent dimentions.")
    return fm, D, sigma2_arg(postfilter, D)


def _vc_dev(c, fm, postfilter, delta, call):
    """vc of a trajectory converter on a device tensor fm ((D+1,T) static or (2D+1,T), unit stride along the rows):
    call(ptr, ld, T, is_static, sigma2, out_ptr, ld_out, stream) is the converter's `_dev` entry; the result is the (D+1,T)
    transposed view of a new (T, D+1) device buffer, like push_delta's."""
    import torch

    ptr, rows, T, ld = dev_matrix(fm, "fm")
    D = c._static_dim()
    if rows != (D if delta else c._dim()) + 1:
        raise _lib.DimensionMismatch("Inconsistent dimentions.")
    s2 = sigma2_arg(postfilter, D)
    buf = torch.empty((T, D + 1), dtype=torch.float64, device=fm.device)
    _lib.check(call(ptr, ld, T, int(bool(delta)), s2, buf.data_ptr(), D + 1, current_stream_ptr()))
    return buf.t()


def _vc_batch(c, fms, postfilter, delta, host_call, dev_call):
    """vc_batch of a trajectory converter.  host_call(n, fm**, T*, is_static, sigma2, out**) and
    dev_call(n, dfm, fm_off*, T*, is_static, sigma2, dout, out_off*, stream) are the converter's two batch entries.  Device
    tensors are addressed where they are, by their offsets from the first one (a tensor that is not dense is copied); the
    results are views of one new (sum T, D+1) buffer."""
    fms = list(fms)
    n = len(fms)
    if n == 0:
        return []
    D = c._static_dim()
    rows = (D if delta else c._dim()) + 1
    on_dev = [is_torch(f) and f.is_cuda for f in fms]
    if any(on_dev) and not all(on_dev):
        raise TypeError("vc_batch: device tensors and host matrices in one list")
    if not on_dev[0]:
        fms = [jl_matrix(f, "fm") for f in fms]
    for f in fms:
        if f.shape[0] != rows:
            raise _lib.DimensionMismatch("Inconsistent dimentions.")
    s2 = sigma2_arg(postfilter, D)
    T = np.array([f.shape[1] for f in fms], dtype=np.int64)
    if not on_dev[0]:
        outs = [np.empty((D + 1, int(t)), order="F") for t in T]
        dpp = C.POINTER(C.c_double) * n
        _lib.check(host_call(n, dpp(*[_lib.dptr(f) for f in fms]), _lib.iptr(T), int(bool(delta)), s2,
                             dpp(*[_lib.dptr(o) for o in outs])))
        return outs
    import torch

    dense = []                                   # (kept alive until the call returns: it ends with a status read)
    for f in fms:
        if f.shape[1] > 0:                       # (an empty tensor has no strides to speak of, and is never read)
            _, _, t, ld = dev_matrix(f, "fm")
            if t > 1 and ld != rows:
                f = f.t().contiguous().t()
        dense.append(f)
    ptrs = [f.data_ptr() for f in dense]
    base = next((p for p, t in zip(ptrs, T) if t > 0), 0)
    fm_off = np.array([(p - base) // 8 if t > 0 else 0 for p, t in zip(ptrs, T)], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(T)])
    buf = torch.empty((int(first[-1]), D + 1), dtype=torch.float64, device=fms[0].device)
    out_off = np.ascontiguousarray(first[:-1] * (D + 1), dtype=np.int64)
    _lib.check(dev_call(n, base, _lib.iptr(fm_off), _lib.iptr(T), int(bool(delta)), s2, buf.data_ptr(), _lib.iptr(out_off),
                        current_stream_ptr()))
    return [buf[int(first[u]):int(first[u + 1])].t() for u in range(n)]


class TrajectoryGMMMap(TrajectoryConverter):
    """TrajectoryGMMMap(g::GMMMap, T) -- src/trajectory_gmmmap.jl:3-37.  `g` is a GMMMap over static+delta
    features (dim(g) = 2D).  The constructor precomputes Dy_m = inv(Sigma^yy_m - A_m Sigma^xy_m) (:24-28)."""

    _PRECISIONS = ("full", "diag")          # VCMI_TRAJ_PRECISION_FULL, VCMI_TRAJ_PRECISION_DIAG

    def __init__(self, g, T, em_iters=0, precision="full"):
        if isinstance(g, BlockDiagGMMMap):
            raise TypeError("TrajectoryGMMMap takes a GMMMap, not a BlockDiagGMMMap: build it from "
                            "GMMMap(weights, mu, expand_block_diag(covars)) (precision=\"diag\" then converts with the model exactly), "
                            "or use BlockDiagTrajectoryGMMMap(g, T), which converts straight from the cross-diagonal model")
        self.gmmmap = g
        h = C.c_void_p()
        _lib.check(_lib.lib.vcmi_traj_create(g._h, int(T), C.byref(h)))
        self._h = h
        if em_iters:
            self.em_iters = em_iters
        if precision != "full":
            self.precision = precision

    @property
    def precision(self):
        """The conditional precisions of the conversion.  "full" (default): Dy_m = inv(Sigma^yy_m - A_m Sigma^xy_m), the
        reference's conversion.  "diag": the conditional covariance of every mixture taken as diagonal, as MLPG is commonly
        run -- the normal equations fall apart into tridiagonal systems per static dimension and frame parity, solved in
        O(T D) (csrc/traj_diag.hip).  fvconvert, fvconvert_batch, vc and vc_batch pick the setting up from the converter.
        Not together with em_iters > 0 or under a TrajectoryGVGMMMap (VCMIError; the GV converter over "diag" is
        DiagTrajectoryGVGMMMap); cond_loglik always evaluates the full-covariance model.  EM re-estimation over diagonal
        precisions exists where they are exact: BlockDiagTrajectoryEMGMMMap, over a cross-diagonal model."""
        return self._PRECISIONS[int(_lib.lib.vcmi_traj_get_precision(self._h))]

    @precision.setter
    def precision(self, kind):
        # (a name the library does not know goes to it as a kind it does not know: the refusal is the library's)
        k = self._PRECISIONS.index(kind) if kind in self._PRECISIONS else -1
        _lib.check(_lib.lib.vcmi_traj_set_precision(self._h, k))

    @property
    def em_iters(self):
        """EM iterations after the arg-max solution (Toda et al. 2007, eqs. 30-36: every mixture weighted by
        P(m | X_t, Y_t)) instead of the suboptimum mixture sequence of src/trajectory_gmmmap.jl:81-82 alone.  0 (default):
        the reference's conversion.  fvconvert, fvconvert_batch and vc pick the setting up from the converter."""
        return int(_lib.lib.vcmi_traj_get_em(self._h))

    @em_iters.setter
    def em_iters(self, n):
        _lib.check(_lib.lib.vcmi_traj_set_em(self._h, int(n)))

    _cond_loglik = staticmethod(_lib.lib.vcmi_traj_cond_loglik)
    _cond_loglik_dev = staticmethod(_lib.lib.vcmi_traj_cond_loglik_dev)

    def cond_loglik(self, X, Y):
        """L(y) = log P(W y | X) for one utterance, X (2D,T), Y (D,T): the objective the EM iterations raise.  numpy
        matrices give a float; device tensors (dense, unit stride along the features) a one-element device tensor."""
        if is_torch(X) and X.is_cuda:
            import torch

            xp, D2, T, ldx = dev_matrix(X, "X")
            yp, D, Ty, ldy = dev_matrix(Y, "Y")
            if D2 != self._dim() or D != self._static_dim() or Ty != T:
                raise _lib.DimensionMismatch("Inconsistent dimentions.")
            if T > 1 and (ldx != D2 or ldy != D):
                raise ValueError("cond_loglik: X and Y must be dense")
            out = torch.empty(1, dtype=torch.float64, device=X.device)
            _lib.check(self._cond_loglik_dev(self._h, xp, yp, T, out.data_ptr(), current_stream_ptr()))
            return out
        X, Y = jl_matrix(X, "X"), jl_matrix(Y, "Y")
        if X.shape[0] != self._dim() or Y.shape[0] != self._static_dim() or X.shape[1] != Y.shape[1]:
            raise _lib.DimensionMismatch("Inconsistent dimentions.")
        L = C.c_double(0.0)
        _lib.check(self._cond_loglik(self._h, _lib.dptr(X), _lib.dptr(Y), X.shape[1], C.byref(L)))
        return float(L.value)

    def em_history(self):
        """L(y^k), k = 0 .. n-1: the objective at each E-step of the LAST conversion call (n = the iterations that call ran,
        whatever em_iters is now), summed over its utterances."""
        cap = max(self.em_iters, 1024)
        L = np.empty(cap)
        _lib.check(_lib.lib.vcmi_traj_em_history(self._h, _lib.dptr(L), cap))
        bad = np.flatnonzero(np.isnan(L))           # entries beyond that call's iterations are NaN
        return L[:bad[0]] if len(bad) else L

    def __del__(self, _destroy=_lib.lib.vcmi_traj_destroy):       # bound at definition: module globals may be gone at exit
        h = getattr(self, "_h", None)
        if h:
            _destroy(h)
            self._h = None

    def __len__(self):                      # Base.length(t) = size(W,2) / (dim/2) = T, src/trajectory_gmmmap.jl:34
        return int(_lib.lib.vcmi_traj_length(self._h))

    def _dim(self):                         # src/trajectory_gmmmap.jl:35
        return self.gmmmap._dim()

    @property
    def windows(self):
        """rows of W per frame and static dimension: 2 (static + delta, the reference's), or 3 (static + delta + delta-delta)
        for a BlockDiagTrajectoryGMMMap(g, T, windows=3)"""
        return int(_lib.lib.vcmi_traj_get_windows(self._h))

    def _static_dim(self):                  # D: dim(t) / windows
        return self._dim() // self.windows

    def _ncomponents(self):                 # src/trajectory_gmmmap.jl:36
        return self.gmmmap._ncomponents()

    def _fvconvert(self, X):
        """fvconvert(tgmm, X (2D,T)) -> (D,T); src/trajectory_gmmmap.jl:65-110.  A torch tensor on the device is converted where it
        is and a device tensor comes back (through the batch entry, which leaves len(t) as it is)."""
        if is_torch(X) and X.is_cuda:
            return self.fvconvert_batch([X])[0]
        X = jl_matrix(X, "X")
        D2, T = X.shape
        if D2 != self._dim():               # src/trajectory_gmmmap.jl:68
            raise _lib.DimensionMismatch("Inconsistent dimentions.")
        Y = np.empty((self._static_dim(), T), order="F")
        _lib.check(_lib.lib.vcmi_traj_convert(self._h, _lib.dptr(X), T, _lib.dptr(Y)))
        return Y

    def fvconvert_batch(self, Xs):
        """Batch extension: independent utterances in one launch (one workgroup per utterance).  A list of device tensors (each
        with unit stride along its rows; one that is not dense is copied) is converted where it is, on the current stream
        (vcmi_traj_convert_batch_dev): the results are device tensors, views of one new (sum T, D) buffer."""
        n = len(Xs)
        if n == 0:
            return []
        on_dev = [is_torch(x) and x.is_cuda for x in Xs]
        if any(on_dev):
            if not all(on_dev):
                raise TypeError("fvconvert_batch: device tensors and host matrices in one list")
            return self._fvconvert_batch_dev(list(Xs))
        Xs = [jl_matrix(x, "X") for x in Xs]
        D2 = self._dim()
        for x in Xs:
            if x.shape[0] != D2:
                raise _lib.DimensionMismatch("Inconsistent dimentions.")
        T = np.array([x.shape[1] for x in Xs], dtype=np.int64)
        Ys = [np.empty((self._static_dim(), int(t)), order="F") for t in T]
        dpp = C.POINTER(C.c_double) * n
        _lib.check(_lib.lib.vcmi_traj_convert_batch(self._h, n, dpp(*[_lib.dptr(x) for x in Xs]), _lib.iptr(T),
                                                    dpp(*[_lib.dptr(y) for y in Ys])))
        return Ys

    def _fvconvert_batch_dev(self, Xs):
        import torch

        D2, D = self._dim(), self._static_dim()
        dense = []                                   # (kept alive until the call returns: it ends with a status read)
        for x in Xs:
            if x.dim() != 2 or x.shape[0] != D2:
                raise _lib.DimensionMismatch("Inconsistent dimentions.")
            if x.shape[1] > 0:                       # (an empty tensor has no strides to speak of, and is never read)
                _, _, t, ld = dev_matrix(x, "X")
                if t > 1 and ld != D2:
                    x = x.t().contiguous().t()
            dense.append(x)
        T = np.array([x.shape[1] for x in dense], dtype=np.int64)
        ptrs = [x.data_ptr() for x in dense]
        base = next((p for p, t in zip(ptrs, T) if t > 0), 0)
        x_off = np.array([(p - base) // 8 if t > 0 else 0 for p, t in zip(ptrs, T)], dtype=np.int64)
        first = np.concatenate([[0], np.cumsum(T)])
        buf = torch.empty((int(first[-1]), D), dtype=torch.float64, device=Xs[0].device)
        y_off = np.ascontiguousarray(first[:-1] * D, dtype=np.int64)
        _lib.check(_lib.lib.vcmi_traj_convert_batch_dev(self._h, len(dense), base, _lib.iptr(x_off), _lib.iptr(T), buf.data_ptr(),
                                                        _lib.iptr(y_off), current_stream_ptr()))
        return [buf[int(first[u]):int(first[u + 1])].t() for u in range(len(dense))]

    def _vc(self, fm, postfilter=None, delta=False):
        """vc(c::TrajectoryConverter, fm (2D+1,T)) -> (D+1,T) in chunks of length(c) frames; src/common.jl:31-63.
        delta=True: fm holds STATIC features (D+1,T); the deltas are taken on the device over the whole matrix before it is
        cut into chunks (bin/vc.jl:75-78; vcmi_vc_traj_static).  A torch tensor on the device is converted where it is, on
        the current stream (vcmi_vc_traj_dev), and a device tensor (D+1,T) comes back."""
        if is_torch(fm) and fm.is_cuda:
            def entry(*args):
                return _lib.lib.vcmi_vc_traj_dev(self._h, *args)

            return _vc_dev(self, fm, postfilter, delta, entry)
        fm, D, s2 = _vc_host_args(self, fm, postfilter, delta)
        out = np.empty((D + 1, fm.shape[1]), order="F")
        entry = _lib.lib.vcmi_vc_traj_static if delta else _lib.lib.vcmi_vc_traj_postf      # (NULL sigma2: vcmi_vc_traj)
        _lib.check(entry(self._h, _lib.dptr(fm), fm.shape[1], s2, _lib.dptr(out)))
        return out

    def _vc_batch(self, fms, postfilter=None, delta=False):
        """vc_batch (common.py): vcmi_vc_traj_batch on host matrices, vcmi_vc_traj_batch_dev on device tensors"""
        def host(*args):
            return _lib.lib.vcmi_vc_traj_batch(self._h, *args)

        def dev(*args):
            return _lib.lib.vcmi_vc_traj_batch_dev(self._h, *args)

        return _vc_batch(self, fms, postfilter, delta, host, dev)


class BlockDiagTrajectoryGMMMap(TrajectoryGMMMap):
    """BlockDiagTrajectoryGMMMap(g::BlockDiagGMMMap, T): trajectory conversion straight from a cross-diagonal model over
    static+delta features (dim(g) = 2D) -- what train_gmm(covariance_type="block_diag") returns, as it is.  The conditional
    covariance of such a model is diagonal exactly, so the converter runs the tridiagonal solver of precision="diag" and the dense
    (4D,4D,M) model is never formed (include/vcmi.h: vcmi_traj_create_bdiag; csrc/gmmmap_bdiag.hip, mode 3).  Equal to
    TrajectoryGMMMap(GMMMap(weights, mu, expand_block_diag(covars)), T, precision="diag") to rounding.  fvconvert,
    fvconvert_batch, vc and vc_batch are TrajectoryGMMMap's; precision is "diag" for good, and em_iters > 0, precision = "full",
    cond_loglik and a TrajectoryGVGMMMap over it are refused (VCMIError); global variance: DiagTrajectoryGVGMMMap.  Converts on the
    device g was created on.  EM re-estimation over all mixtures and cond_loglik for such a model: BlockDiagTrajectoryEMGMMMap.
    windows=3: g is a model over static + delta + delta-delta features (dim(g) = 3D, the rows push_delta(src, order=2) makes;
    DimensionMismatch otherwise; VCMIError for any other count).  W = constructW(D, T, windows=3), and the normal
    equations are one pentadiagonal system per static dimension (csrc/traj_penta.hip; include/vcmi.h:
    vcmi_traj_create_bdiag_windows).  fvconvert, fvconvert_batch and vc(c, fm (3D+1,T)) with or without a postfilter, on host
    matrices and (vc) device tensors, convert with it; vc(..., delta=True), vc_batch, BlockDiagTrajectoryEMGMMMap's em_iters > 0 and
    cond_loglik, and a DiagTrajectoryGVGMMMap over it are refused (VCMIError naming three windows): follow-ups.  Global variance
    over three windows: BlockDiagTrajectoryGVGMMMap."""

    def __init__(self, g, T, windows=2):
        if not isinstance(g, BlockDiagGMMMap):
            raise TypeError(f"BlockDiagTrajectoryGMMMap takes a BlockDiagGMMMap, not a {type(g).__name__}")
        if isinstance(windows, bool) or not isinstance(windows, (int, np.integer)):
            raise TypeError(f"BlockDiagTrajectoryGMMMap: windows must be an integer, not a {type(windows).__name__}")
        self.gmmmap = g                     # (kept alive: the library's handle reads g's tables in every call)
        h = C.c_void_p()
        if windows == 2:                    # (the entry the converter has always used)
            _lib.check(_lib.lib.vcmi_traj_create_bdiag(g._h, int(T), C.byref(h)))
        else:
            _lib.check(_lib.lib.vcmi_traj_create_bdiag_windows(g._h, int(T), int(windows), C.byref(h)))
        self._h = h


class BlockDiagTrajectoryEMGMMMap(BlockDiagTrajectoryGMMMap):
    """BlockDiagTrajectoryEMGMMMap(g::BlockDiagGMMMap, T, em_iters=1): BlockDiagTrajectoryGMMMap with EM re-estimation over ALL
    mixtures (Toda et al. 2007, eqs. 30-36: every mixture weighted by P(m | X_t, Y_t)) after the arg-max solution, in closed
    form from the cross-diagonal parameters: the blended precision of a frame is a vector of 2D doubles and every M-step is the
    tridiagonal solve again (include/vcmi.h: vcmi_traj_set_em_bdiag; csrc/traj_em_bdiag.hip).  Equal to
    TrajectoryGMMMap(GMMMap(weights, mu, expand_block_diag(covars)), T, em_iters=n) to rounding.  em_iters may be changed at any
    time (0: BlockDiagTrajectoryGMMMap's conversion, launch for launch); cond_loglik evaluates L(y) = log P(W y | X); fvconvert,
    fvconvert_batch, vc, vc_batch and em_history are inherited.  A DiagTrajectoryGVGMMMap over it converts only while
    em_iters == 0 (VCMIError otherwise)."""

    _cond_loglik = staticmethod(_lib.lib.vcmi_traj_cond_loglik_bdiag)
    _cond_loglik_dev = staticmethod(_lib.lib.vcmi_traj_cond_loglik_bdiag_dev)

    def __init__(self, g, T, em_iters=1):
        super().__init__(g, T)
        self.em_iters = em_iters

    @property
    def em_iters(self):
        """EM iterations after the arg-max solution; 0: the conversion of BlockDiagTrajectoryGMMMap"""
        return int(_lib.lib.vcmi_traj_get_em(self._h))

    @em_iters.setter
    def em_iters(self, n):
        _lib.check(_lib.lib.vcmi_traj_set_em_bdiag(self._h, int(n)))


class TrajectoryGVGMMMap(TrajectoryConverter):
    """TrajectoryGVGMMMap(tgmm, mu^v, Sigma^vv) -- src/trajectory_gmmmap.jl:114-137: trajectory conversion followed
    by gradient ascent on the likelihood that includes the global variance (Toda et al. 2007, eqs. (52), (58))."""

    _create = staticmethod(_lib.lib.vcmi_trajgv_create)

    def __init__(self, tgmm, muv, sigmavv):
        muv = np.ascontiguousarray(np.asarray(muv, dtype=np.float64).reshape(-1))
        sigmavv = jl_matrix(sigmavv, "sigmavv")
        D = tgmm._static_dim()
        if muv.shape != (D,) or sigmavv.shape != (D, D):
            raise _lib.DimensionMismatch("the GV statistics must have the static feature dimension")
        if np.any(muv < 0):                 # @assert sum(mu^v .< 0) == 0, src/trajectory_gmmmap.jl:124
            raise AssertionError("the GV mean must be non-negative")
        self.tgmm = tgmm
        h = C.c_void_p()
        _lib.check(self._create(tgmm._h, _lib.dptr(muv), _lib.dptr(sigmavv), C.byref(h)))
        self._h = h

    def __del__(self, _destroy=_lib.lib.vcmi_trajgv_destroy):     # bound at definition: module globals may be gone at exit
        h = getattr(self, "_h", None)
        if h:
            _destroy(h)
            self._h = None

    def __len__(self):                      # src/trajectory_gmmmap.jl:132
        return len(self.tgmm)

    def _dim(self):                         # :133
        return self.tgmm._dim()

    def _static_dim(self):
        return self.tgmm._static_dim()

    def _ncomponents(self):                 # :134
        return self.tgmm._ncomponents()

    def _fvconvert(self, X, epochs=100, alpha=1.0e-5, verbose=False):
        """fvconvert(tgv, X (2D,T); epochs=100, alpha=1.0e-5) -> (D,T); src/trajectory_gmmmap.jl:139-168"""
        return self.fvconvert_batch([X], epochs=epochs, alpha=alpha)[0]

    def fvconvert_batch(self, Xs, epochs=100, alpha=1.0e-5):
        n = len(Xs)
        if n == 0:
            return []
        Xs = [jl_matrix(x, "X") for x in Xs]
        D2 = self._dim()
        for x in Xs:
            if x.shape[0] != D2:
                raise _lib.DimensionMismatch("Inconsistent dimentions.")
        T = np.array([x.shape[1] for x in Xs], dtype=np.int64)
        Ys = [np.empty((self._static_dim(), int(t)), order="F") for t in T]
        dpp = C.POINTER(C.c_double) * n
        _lib.check(_lib.lib.vcmi_trajgv_convert_batch(self._h, n, dpp(*[_lib.dptr(x) for x in Xs]), _lib.iptr(T), int(epochs),
                                                      float(alpha), dpp(*[_lib.dptr(y) for y in Ys])))
        return Ys

    def _vc(self, fm, postfilter=None, delta=False, epochs=100, alpha=1.0e-5):
        """vc(c::TrajectoryConverter, fm): chunks of length(c) frames, each converted with fvconvert(tgv, X; epochs, alpha);
        src/common.jl:31-63.  A postfilter, delta=True (STATIC features (D+1,T), deltas over the whole matrix first:
        bin/vc.jl:75-78), a device tensor or non-default epochs / alpha run as one call on the device (vcmi_vc_trajgv,
        vcmi_vc_trajgv_dev), after which len(c) is the last chunk's length as the reference leaves it
        (src/trajectory_gmmmap.jl:70-72,146).  The plain call on a host matrix keeps the loop below."""
        if is_torch(fm) and fm.is_cuda:
            def entry(ptr, ld, T, is_static, s2, optr, ldo, stream):
                return _lib.lib.vcmi_vc_trajgv_dev(self._h, ptr, ld, T, is_static, int(epochs), float(alpha), s2, optr, ldo, stream)

            return _vc_dev(self, fm, postfilter, delta, entry)
        if delta or postfilter is not None or (epochs, alpha) != (100, 1.0e-5):
            fm, D, s2 = _vc_host_args(self, fm, postfilter, delta)
            out = np.empty((D + 1, fm.shape[1]), order="F")
            _lib.check(_lib.lib.vcmi_vc_trajgv(self._h, _lib.dptr(fm), fm.shape[1], int(bool(delta)), int(epochs), float(alpha), s2,
                                               _lib.dptr(out)))
            return out
        # (not vcmi_vc_trajgv: this loop shards over a device group and leaves len(c) alone)
        fm, D, _ = _vc_host_args(self, fm, None, False)
        T, L = fm.shape[1], len(self)
        out = np.empty((D + 1, T), order="F")
        chunks = [np.asfortranarray(fm[1:, b:min(b + L, T)]) for b in range(0, T, L)]
        for k, y in enumerate(self.fvconvert_batch(chunks)):
            out[1:, k * L:k * L + y.shape[1]] = y
        out[0, :] = fm[0, :]
        return out

    def _vc_batch(self, fms, postfilter=None, delta=False, epochs=100, alpha=1.0e-5):
        """vc_batch (common.py): every chunk of every utterance through fvconvert(tgv, X; epochs, alpha)"""
        def host(n, fm, T, is_static, s2, out):
            return _lib.lib.vcmi_vc_trajgv_batch(self._h, n, fm, T, is_static, int(epochs), float(alpha), s2, out)

        def dev(n, dfm, fm_off, T, is_static, s2, dout, out_off, stream):
            return _lib.lib.vcmi_vc_trajgv_batch_dev(self._h, n, dfm, fm_off, T, is_static, int(epochs), float(alpha), s2, dout,
                                                     out_off, stream)

        return _vc_batch(self, fms, postfilter, delta, host, dev)


class DiagTrajectoryGVGMMMap(TrajectoryGVGMMMap):
    """DiagTrajectoryGVGMMMap(tgmm, mu^v, Sigma^vv): the global-variance conversion of TrajectoryGVGMMMap over a converter with
    DIAGONAL conditional precisions -- a TrajectoryGMMMap(precision="diag") or a BlockDiagTrajectoryGMMMap.  The likelihood
    gradient of the ascent is then a three-point stencil per static dimension, O(T D) per epoch (csrc/traj_gv_band.hip;
    include/vcmi.h: vcmi_trajgv_create_diag).  fvconvert, fvconvert_batch, vc and vc_batch are TrajectoryGVGMMMap's.  The
    converter must have precision "diag" when this is made and whenever it converts (VCMIError otherwise; usable again after
    the switch back); a TrajectoryGVGMMMap over the same converter keeps refusing while the precision is "diag"."""

    _create = staticmethod(_lib.lib.vcmi_trajgv_create_diag)


class BlockDiagTrajectoryGVGMMMap(DiagTrajectoryGVGMMMap):
    """BlockDiagTrajectoryGVGMMMap(tgmm, mu^v, Sigma^vv): the global-variance conversion over a BlockDiagTrajectoryGMMMap
    (TypeError for any other tgmm), through an entry of its own (include/vcmi.h: vcmi_trajgv_create_bdiag).  Two windows: a
    DiagTrajectoryGVGMMMap bit for bit.  windows=3, which DiagTrajectoryGVGMMMap keeps refusing: the likelihood gradient is the
    five-point stencil of the pentadiagonal system the converter solves, a Jacobi step per epoch (csrc/traj_gv_band.hip).
    fvconvert and fvconvert_batch take X (3D,T); vc takes fm (3D+1,T), host matrix or device tensor, with or without a
    postfilter.  delta=True and vc_batch over three windows stay refused (VCMIError naming three windows)."""

    _create = staticmethod(_lib.lib.vcmi_trajgv_create_bdiag)

    def __init__(self, tgmm, muv, sigmavv):
        if not isinstance(tgmm, BlockDiagTrajectoryGMMMap):
            raise TypeError(f"BlockDiagTrajectoryGVGMMMap: tgmm must be a BlockDiagTrajectoryGMMMap, not a {type(tgmm).__name__}")
        super().__init__(tgmm, muv, sigmavv)
