"""Type hierarchy and the `vc` batch drivers -- reference src/common.jl:1-63."""


class AbstractConverter:            # src/common.jl:2
    pass


class FrameByFrameConverter(AbstractConverter):   # src/common.jl:3
    pass


class TrajectoryConverter(AbstractConverter):     # src/common.jl:4
    pass


def vc(c, fm, postfilter=None, delta=False):
    """vc(c, fm): row 1 of `fm` is the power coefficient and is passed through; the remaining rows are
    converted -- frame by frame for a FrameByFrameConverter (src/common.jl:7-26; here one kernel launch
    over all T frames), in chunks of length(c) frames for a TrajectoryConverter (src/common.jl:31-63).
    postfilter: a VarianceScaling applied to the converted rows 2..end before the result leaves the device
    (out[2:end,:] = fvpostf(postfilter, vc(c, fm)[2:end,:]), src/gv.jl:10-15): one upload, one download.
    delta=True (TrajectoryConverter only, as bin/vc.jl:76): `fm` holds the STATIC features (D+1,T) and the input
    [fm[1,:]; push_delta(fm[2:end,:])] of bin/vc.jl:77-78 is built on the device -- the deltas over the whole
    utterance, before it is cut into chunks.  A trajectory converter also takes a torch tensor on the device
    and returns one."""
    if delta:
        if isinstance(c, FrameByFrameConverter):
            raise ValueError("delta=True: only a TrajectoryConverter takes delta features (bin/vc.jl:76)")
        return c._vc(fm, postfilter, delta=True)
    if postfilter is None:
        return c._vc(fm)
    return c._vc(fm, postfilter)


def vc_batch(c, fms, postfilter=None, delta=False, **kw):
    """vc over a whole list of utterances in one call: vc_batch(c, fms, postfilter, delta, ...)[u] is what
    vc(c_u, fms[u], postfilter, delta, ...) returns for a fresh converter c_u equal to `c` with len(c_u) = len(c) -- chunks of
    len(c) frames per utterance, deltas (delta=True) and the post-filter's statistics over that utterance only, the power row
    passed through -- with one upload, one trajectory solve over the chunks of all utterances and one download
    (include/vcmi.h: vcmi_vc_traj_batch).  Unlike vc, the call leaves len(c) unchanged.
    fms: a list of (rows, T_u) matrices, T_u = 0 allowed; the result is a list of Fortran (D+1, T_u) arrays.  A trajectory
    converter also takes a list of device tensors (each with unit stride along its rows) and returns device tensors, views of
    one buffer, on the current stream.  **kw: epochs / alpha of a TrajectoryGVGMMMap."""
    if delta and isinstance(c, FrameByFrameConverter):
        raise ValueError("delta=True: only a TrajectoryConverter takes delta features (bin/vc.jl:76)")
    if isinstance(c, FrameByFrameConverter):
        return c._vc_batch(fms, postfilter, **kw)
    return c._vc_batch(fms, postfilter, delta, **kw)


def fvconvert(c, x, **kw):
    """fvconvert(c, x): src/gmmmap.jl:101-118 (vector or, as a batch extension, (D,T) matrix) and
    src/trajectory_gmmmap.jl:65-110 ((2D,T) matrix)."""
    return c._fvconvert(x, **kw)


def dim(c):
    return c._dim()


def ncomponents(c):
    return c._ncomponents()


def size(c):
    return (dim(c), len(c))
