"""Call histories (test helper, not a test module; nothing here touches the GPU at import).

The library keeps device and pinned memory between calls: on the handles (grouping buffers and their two ping-pong
super-chunk tables, scratch_lp, the trajectory workspaces and status word) and per host thread (E-step, mgc, DTW, dataset,
post-filter and vc scratch) -- DESIGN.md, "State that outlives a call".  A test of that state runs a SEQUENCE of calls on
shared handles in one thread (`play`) and compares every step, bit for bit, with the same single call in the fresh state:
a new thread, whose thread_local scratch is new, and a new handle (`fresh`).

One rule for every sequence: consecutive calls get DIFFERENT frames (disjoint slices of one seeded draw, `slices`).  With
equal frames a stale key, permutation or statistic is the right one and the test is blind.

The sequences themselves are module-level data, so that tests/test_call_history_host.py can prove without a GPU that the
chosen sizes reach the state changes the GPU tests claim."""
import threading

import numpy as np

# ---- csrc constants restated (tests/test_call_history_host.py reads them back from the sources) ----
GROUP_CHUNK = 1024          # kGroupChunk, csrc/grouping.hpp
SORT_MIN_FRAMES = 8192      # kSortMinFrames, csrc/gmmmap_group.hip: calls from here on are grouped


def fresh(fn):
    """fn() in a new thread (new thread_local scratch; fn builds its own handles): its result, or its exception re-raised.
    Joining the thread also runs the scratch destructors (hipFree, hipEventDestroy) while the caller's thread goes on."""
    box = {}

    def run():
        box["tid"] = threading.get_ident()
        try:
            box["result"] = fn()
        except BaseException as e:  # noqa: BLE001  (re-raised in the caller)
            box["error"] = e

    t = threading.Thread(target=run)
    t.start()
    t.join()
    fresh.last_thread_id = box.get("tid")
    if "error" in box:
        raise box["error"]
    return box["result"]


fresh.last_thread_id = None


def to_numpy(r):
    """Results as host numpy arrays (device tensors are downloaded, which also waits for them); tuples / lists element-wise."""
    if isinstance(r, (tuple, list)):
        return tuple(to_numpy(x) for x in r)
    if type(r).__module__.split(".")[0] == "torch":
        return r.detach().cpu().numpy().copy()
    return np.array(r, copy=True)


def play(steps):
    """Run [(name, fn), ...] in order in the calling thread (the fns share handles); {name: result as numpy}."""
    out = {}
    for name, fn in steps:
        assert name not in out, f"duplicate step name {name}"
        out[name] = to_numpy(fn())
    return out


def same_bits(a, b):
    """Bit equality of two results of to_numpy (NaN payloads included)."""
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def grouping_geometry(T, M):
    """launch_grouping (csrc/gmmmap_group.hip) restated: chunks of 1024 frames, 2^shift chunks per super-chunk (the power of two
    from 32 on that reaches sqrt(nchunks)), nsuper super-chunks, and the ints one super-chunk table needs."""
    nchunks = (T + GROUP_CHUNK - 1) // GROUP_CHUNK
    shift = 5
    while (1 << (2 * shift)) < nchunks:
        shift += 1
    nsuper = (nchunks + (1 << shift) - 1) >> shift
    return {"nchunks": nchunks, "shift": shift, "nsuper": nsuper, "table_ints": nsuper * M}


def grouped(op, T, predict_screens):
    """Does this step go through launch_grouping (and so advance grp_calls)?  fvconvert from 8192 frames on; predict as
    well where the model lets the screened arg-max pay (the peaked synthetic model); predict_proba never."""
    if T < SORT_MIN_FRAMES:
        return False
    return op == "convert" or (op == "predict" and predict_screens)


def slices(lengths):
    """Disjoint [start, stop) slices of one draw, in order: consecutive calls never see the same frames."""
    out, at = [], 0
    for n in lengths:
        out.append((at, at + n))
        at += n
    return out


# ---- 3a. one GMMMap, many sizes -------------------------------------------------------------------------------------
# grouped sizes visit nsuper = 1, 2, 1, 3 (the tables are allocated, reused by a smaller call, reallocated), 100 / 1 / 8191
# stay under the grouping threshold, 8192 is the threshold itself, 8209 and 40 000 come twice
FVCONVERT_T = [8209, 100, 40_000, 8192, 70_001, 1, 8209, 40_000, 8191]
_PATTERN = ["convert", "predict", "convert", "posterior"]
# the same list with predict and predict_proba in between, once in each phase of the pattern, and a tail that puts the
# screened arg-max on the odd table as well
INTERLEAVED = ([(_PATTERN[i % 4], T) for i, T in enumerate(FVCONVERT_T)] +
               [(_PATTERN[(i + 1) % 4], T) for i, T in enumerate(FVCONVERT_T)] +
               [("convert", 40_000), ("predict", 8209)])
# host-pointer entry: the same sizes, then one call long enough for the staging ring (several chunks of kMinChunkFrames =
# 98304 frames), then two that skip it
HOST_T = FVCONVERT_T + [300_001, 1, 2000]
# D = 16, M = 4: more than 1024 chunks -> group_super_shift 6; then a small grouped call (shift 5); then the long one again
LONG_T = [1_050_000, 8193, 1_050_000]
# prune / kernel toggles: (setting, T); every call other frames
TOGGLES = [("prune_inf", 8209), ("prune_46", 8209), ("kernel_1", 3000), ("kernel_0", 8209)]

# ---- 3d. thread-local scratch across shapes ---------------------------------------------------------------------------
ESTEP_DIAG_SHAPES = [(70_000, 80, 128, "apart"), (31, 80, 128, "apart"), (4000, 80, 16, "apart"), (3000, 48, 128, "apart"),
                     (2000, 79, 20, "apart"), (70_000, 80, 128, "overlap")]
ESTEP_FULL_SHAPES = [(20_000, 80, 64), (1, 80, 3), (5000, 160, 6), (1500, 48, 8)]
MGC_A, MGC_B, MGC_C = (41, 0.41, 1024), (25, 0.58, 512), (41, 0.42, 1024)
MGC_SHAPES = [("A1", MGC_A), ("B", MGC_B), ("A2", MGC_A), ("C", MGC_C), ("A3", MGC_A)]
POSTF_SHAPES = [(40, 300_001), (7, 3), (256, 50)]


def sequence_frames(seq):
    """(name, op, T, (start, stop)) for a sequence of (op, T): the slice of the sequence's one draw that each step reads."""
    sl = slices([T for _, T in seq])
    return [(f"{i:02d}_{op}_{T}", op, T, s) for i, ((op, T), s) in enumerate(zip(seq, sl))]
