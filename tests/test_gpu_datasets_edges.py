"""GPU: csrc/dataset.hip at its edges -- mc2e at the fft lengths the reference pipeline uses (1024 / 2048 / 4096: more dynamic LDS
than the default limit, fewer frames per workgroup), the grid-stride pass of mc2e_kernel, frames placed ON the silence threshold,
keep patterns dictated across every seam of keep_index_kernel's compaction, pairs that keep 0 / 1 / 2 frames, and the grow-only
scratch.  References: the C oracle (mc2e, align_mcep, joint_features) and, for mc2e, the frequency-domain evaluation of
oracle/crosscheck.py; the dictated patterns are also checked by plain numpy indexing.  Values are copies / exact halves, so the
matrices are compared bit for bit; mc2e holds the tolerances of tests/test_gpu_datasets.py::test_mc2e."""
import ctypes as C

import numpy as np
import pytest

import dataset_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def _check_mc2e(vc, mc, alpha, fftlen):
    from oracle import c_oracle as co
    from oracle import crosscheck as cc
    e = vc.mc2e(mc.T, alpha, fftlen)
    ref = co.mc2e(mc, alpha, fftlen)
    e_t, _ = cc.mc2e_frequency_domain(mc, alpha, fftlen)
    err, err_t = np.max(np.abs(e - ref) / ref), np.max(np.abs(e - e_t) / e_t)
    print(f"mc2e D={mc.shape[1]} T={len(mc)} fftlen={fftlen}: vs oracle {err:.2e}, vs frequency domain {err_t:.2e}")
    assert err < 1e-12 and err_t < 1e-11
    return e


@pytest.mark.parametrize("D,T,fftlen,alpha", [
    (25, 6, 1024, 0.41),     # 4 waves x 2 x 1024 doubles: exactly 64 KiB of dynamic LDS
    (41, 5, 2048, 0.55),     # 128 KiB: only with the opt-in above the default limit
    (41, 3, 4096, 0.58),     # two frames per workgroup (four would need 256 KiB)
    (25, 6, 100, 0.41),      # not a multiple of the 64 lanes the sums are strided over
    (25, 4, 3, 0.41),        # len < D and len < 64
    (2, 4, 2, 0.3),          # the smallest legal length
])
def test_mc2e_at_the_pipelines_lengths(vc, D, T, fftlen, alpha):
    _check_mc2e(vc, dc.mcep(np.random.default_rng(fftlen), T, D), alpha, fftlen)


def test_mc2e_second_pass_of_the_grid_stride_loop(vc):
    """2048 workgroups of 4 waves: frames 8192 ... 8196 are the second frame of the first five waves, which reuse their g / h
    slices of the LDS.  Distinct c0 per frame: a value left over from the first pass changes the answer."""
    from oracle import c_oracle as co
    T = 4 * 2048 + 5
    mc = dc.mcep(np.random.default_rng(8), T, 3)
    e = vc.mc2e(mc.T, 0.35, 64)
    err = np.abs(e - co.mc2e(mc, 0.35, 64)) / co.mc2e(mc, 0.35, 64)
    assert np.max(err[8192:]) < 1e-12 and np.max(err[:5]) < 1e-12
    assert np.max(err) < 1e-12


def test_mc2e_bits_do_not_depend_on_frames_per_workgroup(vc):
    """the wave count only decides which frame a wave takes: fftlen = 512 gives the same bits with 4, 2 and 1 frames per workgroup"""
    from voiceconversion_jl_amd import _lib
    mc = dc.mcep(np.random.default_rng(9), 37, 41)
    e4 = _check_mc2e(vc, mc, 0.35, 512)
    for flag in (_lib.DBG_MC2E_TWO_WAVES, _lib.DBG_MC2E_ONE_WAVE):
        _lib.debug_force(flag)
        try:
            e = vc.mc2e(mc.T, 0.35, 512)
        finally:
            _lib.debug_force(0)
        assert np.array_equal(e, e4)


def test_fftlen_4096_through_align_mcep_and_the_limit(vc):
    from oracle import c_oracle as co
    rng = np.random.default_rng(10)
    src = dc.mcep(rng, 60, 25)
    tgt = dc.warped_copy(rng, src, 70)
    s_ref, t_ref = co.align_mcep(src, tgt, 0.41, 4096)
    s, t = vc.align_mcep(src.T, tgt.T, 0.41, 4096)
    assert 0 < s.shape[1] < 60
    assert np.array_equal(s, s_ref.T) and np.array_equal(t, t_ref.T)
    _check_mc2e(vc, src[:2], 0.41, 9600)                         # the longest length: one frame per workgroup, 150 KiB
    for call in (lambda n: vc.mc2e(src.T, 0.41, n), lambda n: vc.align_mcep(src.T, tgt.T, 0.41, n)):
        for n in (9601, 16384):
            with pytest.raises(vc.VCMIError, match="at most 9600"):
                call(n)
    assert np.array_equal(vc.align_mcep(src.T, tgt.T, 0.41, 4096)[0], s_ref.T)      # the refusal left nothing behind


def test_frames_on_the_silence_threshold(vc):
    """frames 1e-9 ... 0.5 either side of the threshold (the preconditions are conditions on the INPUT, asserted with the oracle
    before the device is touched: 1e-9 is 1000 x what a 1e-12 relative error of mc2e moves log e by, so a correct kernel cannot
    flip a frame): align_mcep keeps exactly the frames above it, bit for bit the oracle's result"""
    from oracle import c_oracle as co
    src, tgt, want, got = dc.threshold_case()
    assert np.array_equal(np.sign(got), np.sign(want)) and np.all(np.abs(got) >= dc.MIN_GAP)
    s_ref, t_ref = co.align_mcep(src, tgt, dc.ALPHA, dc.FFTLEN, dc.THRESHOLD)
    s, t = vc.align_mcep(src.T, tgt.T, dc.ALPHA, dc.FFTLEN, dc.THRESHOLD)
    assert s.shape[1] == int((got > 0).sum())
    assert np.array_equal(s, s_ref.T) and np.array_equal(t, t_ref.T)
    assert np.array_equal(s, src[got > 0].T)


def _oracle_joint(src, tgt, alpha, fftlen, ignore0th, add_delta, diff, threshold=dc.THRESHOLD):
    """already aligned pair: silence removal + assembly from the oracle's parts"""
    from oracle import c_oracle as co
    keep = np.log(co.mc2e(src, alpha, fftlen)) > threshold
    return co.joint_features(src[keep], tgt[keep], ignore0th, add_delta, diff)


@pytest.mark.parametrize("S", [63, 64, 65, 255, 256, 257, 513])
def test_dictated_keep_patterns_across_the_compaction_seams(vc, S):
    """align=False, remove_silence=True; one pair per pattern (the empty one between others), frames 0.5 either side of the
    threshold: X is the stack of the source and target columns at exactly the dictated indices"""
    rng = np.random.default_rng(S)
    D = 25
    pats = dc.seam_patterns(rng, S)
    srcs = [dc.dictated(rng, keep, D) for _, keep in pats]
    tgts = [rng.standard_normal((S, D)) for _ in pats]
    ds = vc.ParallelDataset([(s.T, t.T) for s, t in zip(srcs, tgts)], align=False, remove_silence=True, ignore0th=False,
                            add_delta=False, alpha=dc.ALPHA, fftlen=dc.FFTLEN, threshold=dc.THRESHOLD)
    X = ds.X.t().cpu().numpy()
    assert list(ds.counts) == [int(keep.sum()) for _, keep in pats] and len(ds) == sum(int(k.sum()) for _, k in pats)
    o = 0
    for (name, keep), s, t in zip(pats, srcs, tgts):
        k = int(keep.sum())
        assert np.array_equal(X[o:o + k], np.hstack([s[np.flatnonzero(keep)], t[np.flatnonzero(keep)]])), (S, name)
        assert np.array_equal(X[o:o + k], _oracle_joint(s, t, dc.ALPHA, dc.FFTLEN, False, False, False)), (S, name)
        o += k
    assert o == X.shape[0]


COUNTS = [3, 0, 1, 2, 40]
LENGTHS = [50, 30, 70, 45, 90]


def _five_pairs(seed, counts=COUNTS):
    rng = np.random.default_rng(seed)
    srcs = [dc.dictated(rng, dc.keep_with_count(rng, S, k), 25) for S, k in zip(LENGTHS, counts)]
    warped = [dc.warped_copy(rng, s, len(s) + 7) for s in srcs]
    same = [dc.warped_copy(rng, s, len(s)) for s in srcs]
    return srcs, warped, same


def _build(vc, srcs, tgts, align, diff, ignore0th):
    return vc.ParallelDataset([(s.T, t.T) for s, t in zip(srcs, tgts)], diff=diff, ignore0th=ignore0th, add_delta=True,
                              align=align, alpha=dc.ALPHA, fftlen=dc.FFTLEN, threshold=dc.THRESHOLD)


def _oracle_five(srcs, tgts, align, diff, ignore0th):
    from oracle import c_oracle as co
    if not align:
        return [_oracle_joint(s, t, dc.ALPHA, dc.FFTLEN, ignore0th, True, diff) for s, t in zip(srcs, tgts)]
    al = [co.align_mcep(s, t, dc.ALPHA, dc.FFTLEN, dc.THRESHOLD) for s, t in zip(srcs, tgts)]
    return [co.joint_features(a, b, ignore0th, True, diff) for a, b in al]


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("diff,ignore0th", [(False, False), (True, True)])
def test_pairs_that_keep_0_1_2_frames(vc, align, diff, ignore0th):
    """kept counts [3, 0, 1, 2, 40] with add_delta: with 1 or 2 frames every delta is the static copy (no k with
    k >= 1 && k + 1 < n), the empty pair shares its output offset with the next one; then every pair silent"""
    srcs, warped, same = _five_pairs(21)
    tgts = warped if align else same
    ds = _build(vc, srcs, tgts, align, diff, ignore0th)
    refs = _oracle_five(srcs, tgts, align, diff, ignore0th)
    Dj = 2 * (25 - ignore0th) * 2
    assert [r.shape[0] for r in refs] == COUNTS
    assert list(ds.counts) == COUNTS and len(ds) == 46 and tuple(ds.X.shape) == (Dj, 46)
    assert np.array_equal(ds.X.t().cpu().numpy(), np.concatenate(refs, axis=0))
    srcs0, warped0, same0 = _five_pairs(22, counts=[0] * 5)
    ds0 = _build(vc, srcs0, warped0 if align else same0, align, diff, ignore0th)
    assert list(ds0.counts) == [0] * 5 and len(ds0) == 0 and tuple(ds0.X.shape) == (Dj, 0)
    if align:                                       # align_mcep of a silent pair: two empty matrices (bin/align.jl:54 warns)
        s, t = vc.align_mcep(srcs0[0].T, warped0[0].T, dc.ALPHA, dc.FFTLEN, dc.THRESHOLD)
        assert s.shape == (25, 0) and t.shape == (25, 0)


def test_result_does_not_depend_on_earlier_calls(vc):
    """the scratch is grow-only and per thread, the freqt matrix cached on (D, len, alpha): dataset A before and after a larger
    dataset, another len, and -- directly before the second build, so that only alpha differs from the cached key -- the same
    (D, len) with another alpha"""
    from oracle import c_oracle as co
    srcs, warped, _ = _five_pairs(21)
    mcA = np.concatenate(srcs)
    first = _build(vc, srcs, warped, True, False, True)
    XA, countsA = first.X.cpu().numpy().copy(), list(first.counts)
    eA = vc.mc2e(mcA.T, dc.ALPHA, dc.FFTLEN)
    # same (D, len), only alpha changes, in both directions: each call must get its own freqt matrix
    e_other = vc.mc2e(mcA.T, 0.3, dc.FFTLEN)
    ref_other = co.mc2e(mcA, 0.3, dc.FFTLEN)
    assert np.max(np.abs(e_other - ref_other) / ref_other) < 1e-12
    assert np.array_equal(vc.mc2e(mcA.T, dc.ALPHA, dc.FFTLEN), eA)
    rng = np.random.default_rng(23)
    big = [dc.mcep(rng, S, 41) for S in (400, 350, 500, 333, 420, 380, 290, 450)]
    ds = vc.ParallelDataset([(s.T, dc.warped_copy(rng, s, len(s) + 11).T) for s in big], add_delta=True, alpha=0.35, fftlen=512)
    assert 0 < len(ds) < sum(len(s) for s in big)
    vc.mc2e(mcA.T, dc.ALPHA, 128)
    assert np.array_equal(vc.mc2e(mcA.T, 0.3, dc.FFTLEN), e_other)
    again = _build(vc, srcs, warped, True, False, True)          # the cached key is (25, 256, 0.3): only alpha differs
    assert list(again.counts) == countsA == COUNTS
    assert np.array_equal(again.X.cpu().numpy(), XA)
    assert np.array_equal(vc.mc2e(mcA.T, dc.ALPHA, dc.FFTLEN), eA)


def test_argument_errors_leave_the_next_call_intact(vc):
    """what the entry points refuse before any launch; after each refusal a valid call on the same thread is still right"""
    import torch
    from voiceconversion_jl_amd import _lib
    rng = np.random.default_rng(24)
    srcs = [dc.dictated(rng, dc.keep_with_count(rng, S, S // 3), 25) for S in (40, 33)]
    tgts = [rng.standard_normal(s.shape) for s in srcs]
    want = np.concatenate([_oracle_joint(s, t, dc.ALPHA, dc.FFTLEN, True, False, False) for s, t in zip(srcs, tgts)], axis=0)
    pairs = [(s.T, t.T) for s, t in zip(srcs, tgts)]
    kw = dict(align=False, alpha=dc.ALPHA, fftlen=dc.FFTLEN, threshold=dc.THRESHOLD)

    def still_right():
        assert np.array_equal(vc.ParallelDataset(pairs, **kw).X.t().cpu().numpy(), want)

    def too_small_a_buffer():
        n, S = 2, np.array([40, 33], dtype=np.int64)
        fs = [np.asfortranarray(s.T) for s in srcs]
        ft = [np.asfortranarray(t.T) for t in tgts]
        buf = torch.empty(72 * 48, dtype=torch.float64, device="cuda")
        nfr, dpp = np.zeros(1, dtype=np.int64), C.POINTER(C.c_double) * n
        _lib.check(_lib.lib.vcmi_parallel_dataset_dev(n, dpp(*[_lib.dptr(a) for a in fs]), _lib.iptr(S), dpp(*[_lib.dptr(a) for a in ft]),
                                                      _lib.iptr(S), 25, 0, dc.ALPHA, dc.FFTLEN, dc.THRESHOLD, 1, 1, 0, 0, buf.data_ptr(),
                                                      72, _lib.iptr(nfr), None))       # 73 frames go in

    still_right()
    for exc, match, call in [
        (vc.VCMIError, "room for 73 frames", too_small_a_buffer),
        (vc.DimensionMismatch, "not aligned", lambda: vc.ParallelDataset([pairs[0], (srcs[1].T, tgts[1][:-1].T)], **kw)),
        (vc.DimensionMismatch, "share the feature dimension", lambda: vc.ParallelDataset([pairs[0], (srcs[1][:, :24].T, tgts[1][:, :24].T)], **kw)),
        (vc.DimensionMismatch, "too small", lambda: vc.ParallelDataset([(s[:1], t[:1]) for s, t in pairs], ignore0th=True, **kw)),
        (vc.VCMIError, "fft length 1 invalid", lambda: vc.ParallelDataset(pairs, **dict(kw, fftlen=1))),
    ]:
        with pytest.raises(exc, match=match):
            call()
        still_right()
