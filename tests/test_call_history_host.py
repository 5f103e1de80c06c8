"""CPU: the call sequences of tests/call_history.py reach what tests/test_gpu_call_history.py claims for them, and the
helper itself works -- checked without a GPU."""
import os
import re
import threading

import pytest

import call_history as ch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voiceconversion.jl_amd", "csrc")


def _constant(file, name):
    m = re.search(rf"{name}\s*=\s*([0-9]+)", open(os.path.join(CSRC, file)).read())
    assert m, f"{name} not found in {file}"
    return int(m.group(1))


def test_restated_constants_are_the_library_s():
    assert _constant("grouping.hpp", "kGroupChunk") == ch.GROUP_CHUNK
    assert _constant("gmmmap_group.hip", "kSortMinFrames") == ch.SORT_MIN_FRAMES
    src = open(os.path.join(CSRC, "gmmmap_group.hip")).read()
    # group_super_shift: from 5 on, while 2^(2 sh) < nchunks
    assert "int sh = 5;" in src and "while (((int64_t)1 << (2 * sh)) < nchunks) ++sh;" in src


def test_grouping_geometry():
    assert ch.grouping_geometry(8192, 64) == {"nchunks": 8, "shift": 5, "nsuper": 1, "table_ints": 64}
    assert ch.grouping_geometry(1024 * 1024, 4)["shift"] == 5 and ch.grouping_geometry(1024 * 1024, 4)["nsuper"] == 32
    assert ch.grouping_geometry(1024 * 1024 + 1, 4) == {"nchunks": 1025, "shift": 6, "nsuper": 17, "table_ints": 68}


@pytest.mark.parametrize("seq", [[("convert", T) for T in ch.FVCONVERT_T], ch.INTERLEAVED, [("convert", T) for T in ch.HOST_T],
                                 [("convert", T) for T in ch.LONG_T], [("convert", T) for _, T in ch.TOGGLES]])
def test_consecutive_steps_never_share_frames(seq):
    steps = ch.sequence_frames(seq)
    assert len({name for name, *_ in steps}) == len(steps)
    for (_, _, Ta, (a0, a1)), (_, _, Tb, (b0, b1)) in zip(steps, steps[1:]):
        assert a1 - a0 == Ta and b1 - b0 == Tb and a1 <= b0
    # (disjoint throughout, not only between neighbours)
    assert steps[-1][3][1] == sum(T for _, T in seq)


def test_fvconvert_sizes_reallocate_shrink_and_reallocate_the_super_chunk_tables():
    grouped = [T for T in ch.FVCONVERT_T if ch.grouped("convert", T, False)]
    nsuper = [ch.grouping_geometry(T, 64)["nsuper"] for T in grouped]
    assert nsuper[:4] == [1, 2, 1, 3]                 # table grows at 40 000, is reused by 8192, grows again at 70 001
    assert all(ch.grouping_geometry(T, 64)["shift"] == 5 for T in grouped)
    assert 8192 in grouped and 8191 not in grouped and 100 not in grouped and 1 not in grouped   # both sides of the threshold


@pytest.mark.parametrize("predict_screens", [False, True])
def test_interleaved_sequence_uses_both_tables_for_the_repeated_size(predict_screens):
    """grp_calls & 1 selects the table: the repeated T = 8209 converts on both, whether or not the model's predict is the
    screened one (which advances grp_calls too); a screened predict runs on both as well."""
    calls, parity = 0, {}
    for op, T in ch.INTERLEAVED:
        if ch.grouped(op, T, predict_screens):
            parity.setdefault((op, T), set()).add(calls & 1)
            calls += 1
    assert parity[("convert", 8209)] == {0, 1}
    if predict_screens:
        assert set().union(*[p for (op, _), p in parity.items() if op == "predict"]) == {0, 1}
    ops = [op for op, _ in ch.INTERLEAVED]
    assert {"convert", "predict", "posterior"} == set(ops)
    pairs = set(zip(ops, ops[1:]))
    assert {("convert", "predict"), ("predict", "convert"), ("convert", "posterior"), ("posterior", "convert")} <= pairs


def test_long_case_crosses_the_super_shift():
    g = [ch.grouping_geometry(T, 4) for T in ch.LONG_T]
    assert [x["shift"] for x in g] == [6, 5, 6] and g[0]["nchunks"] > 1024
    assert ch.LONG_T[0] == ch.LONG_T[2]              # ... and comes back to it, with other frames (slices)
    assert ch.LONG_T[0] < 1 << 31


def test_mgc_sequence_alternates_shapes_and_alpha():
    names = [n for n, _ in ch.MGC_SHAPES]
    shapes = [s for _, s in ch.MGC_SHAPES]
    assert names == ["A1", "B", "A2", "C", "A3"] and shapes[0] == shapes[2] == shapes[4]
    assert shapes[3][0] == shapes[0][0] and shapes[3][2] == shapes[0][2] and shapes[3][1] != shapes[0][1]   # C: A with another alpha
    assert shapes[1][0] < shapes[0][0] and shapes[1][2] < shapes[0][2]        # B is smaller: rebuilt inside the grow-only buffer


def test_fresh_runs_on_another_thread_and_propagates():
    assert ch.fresh(threading.get_ident) != threading.get_ident()
    assert ch.fresh.last_thread_id != threading.get_ident()
    a, b = ch.fresh(threading.get_ident), ch.fresh(lambda: 7)
    assert b == 7 and isinstance(a, int)

    class Boom(Exception):
        pass

    def bad():
        raise Boom("from the other thread")

    with pytest.raises(Boom, match="from the other thread"):
        ch.fresh(bad)


def test_play_and_same_bits():
    import numpy as np

    out = ch.play([("a", lambda: np.arange(3.0)), ("b", lambda: (np.zeros(2), [1, 2]))])
    assert list(out) == ["a", "b"] and isinstance(out["b"], tuple)
    assert ch.same_bits(out["a"], np.arange(3.0)) and not ch.same_bits(out["a"], np.arange(3))
    assert not ch.same_bits(np.array([0.0]), np.array([-0.0]))            # bits, not values
    assert ch.same_bits(np.array([np.nan]), np.array([np.nan]))
    with pytest.raises(AssertionError):
        ch.play([("a", lambda: 1), ("a", lambda: 2)])
