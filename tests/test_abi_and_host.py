"""CPU: the C-ABI library loads and exports every symbol include/vcmi.h declares; status/exception mapping;
host-side logic of the mirror (no compute calls that need a GPU)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def vc():
    import __graft_entry__ as ge
    ge.build()
    import voiceconversion_jl_amd as m
    return m


def _declared():
    header = open(os.path.join(ROOT, "include", "vcmi.h")).read()
    return sorted(set(re.findall(r"\b(vcmi_[A-Za-z0-9_]+)\s*\(", header)))


def test_every_declared_symbol_is_exported_and_bound(vc):
    from voiceconversion_jl_amd import _lib
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SIGNATURES, f"{n} declared in vcmi.h but not bound in _lib.py"
    assert set(_lib.SIGNATURES) == set(names)
    assert b"gfx950" in _lib.lib.vcmi_version()


def test_no_device_is_reported_not_crashed(vc):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert vc.device_count() == 0
    with pytest.raises(vc.VCMIError, match="no HIP device"):
        vc.GMMMap(np.ones(2) / 2, np.zeros((4, 2)), np.stack([np.eye(4)] * 2, axis=2))
    with pytest.raises(vc.VCMIError):
        vc.fit_(vc.DTW(), np.zeros((2, 3)), np.zeros((2, 3)))


def test_argument_errors_map_to_reference_exceptions(vc):
    with pytest.raises(vc.DimensionMismatch):
        vc.GMMMap(np.ones(3), np.zeros((4, 2)), np.zeros((4, 4, 2)))
    with pytest.raises(vc.DimensionMismatch):
        vc.align(np.zeros((3, 5)), np.zeros((4, 5)))                        # src/align.jl:11-13
    with pytest.raises(vc.DimensionMismatch):
        vc.fit_(vc.DTW(), np.zeros((3, 5)), np.zeros((4, 5)))
    with pytest.raises(vc.DimensionMismatch):
        vc.estep_diag(np.zeros((5, 10)), np.ones(2) / 2, np.zeros((4, 2)), np.ones((4, 2)))


def test_product_does_not_touch_the_oracle():
    """The product package must not import, load or link anything under oracle/."""
    pkg = os.path.join(ROOT, "voiceconversion.jl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".hpp", ".jl")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "vc_oracle" not in text and "np_oracle" not in text and "c_oracle" not in text, os.path.join(dirpath, f)
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), os.path.join(dirpath, f)


@pytest.mark.parametrize("ignore0th,add_delta", [(True, False), (True, True), (False, True), (False, False)])
def test_gv_dataset_host_helper(vc, ignore0th, add_delta):
    """GVDataset (src/datasets.jl:134-183) from in-memory matrices against the numpy restatement: per-utterance corrected
    variances, a single-frame utterance (NaN variance in the reference) skipped, nmax honoured, empty input -> 0 x 0."""
    from oracle import np_oracle as npo
    rng = np.random.default_rng(12)
    fms = [rng.standard_normal((T, 26)) * (1 + i) for i, T in enumerate((50, 1, 333, 2, 17))]
    ds = vc.GVDataset([f.T for f in fms], ignore0th=ignore0th, add_delta=add_delta)
    ref = npo.gv_dataset(fms, ignore0th=ignore0th, add_delta=add_delta)
    assert ds.totalphrases == 5 and ds.X.shape == ref.T.shape == ((26 - ignore0th) * (1 + add_delta), 4)
    assert np.max(np.abs(ds.X - ref.T) / np.abs(ref.T)) < 1e-12
    assert vc.GVDataset([f.T for f in fms], nmax=2).X.shape[1] == 1           # the second utterance has one frame
    assert vc.GVDataset([]).X.shape == (0, 0)
    with pytest.raises(vc.DimensionMismatch):
        vc.GVDataset([fms[0].T, fms[2][:, :5].T])


@pytest.mark.parametrize("add_delta", [False, True])
def test_gv_dataset_short_and_empty_utterances(vc, add_delta):
    """lengths [2, 1, 0, 3, 1]: the one- and zero-frame utterances are skipped (their variance is NaN in the reference), the
    others keep their order, every utterance counts as a phrase; nmax cuts the list BEFORE the skip rule applies"""
    from oracle import np_oracle as npo
    rng = np.random.default_rng(13)
    fms = [rng.standard_normal((T, 6)) * (1 + i) for i, T in enumerate((2, 1, 0, 3, 1))]
    ds = vc.GVDataset([f.T for f in fms], add_delta=add_delta)
    ref = npo.gv_dataset(fms, add_delta=add_delta)
    assert ds.totalphrases == 5 and ds.X.shape == ref.T.shape == (5 * (1 + add_delta), 2)
    assert np.max(np.abs(ds.X - ref.T) / np.abs(ref.T)) < 1e-12
    for k, i in enumerate((0, 3)):                                    # order: utterance 1, then utterance 4
        assert np.allclose(ds.X[:5, k], np.var(fms[i][:, 1:], axis=0, ddof=1), rtol=1e-12, atol=0)
    # nmax = 3 takes [2, 1, 0] and keeps one; skipping first and cutting afterwards would give [2, 3, .] -> two columns
    cut = vc.GVDataset([f.T for f in fms], add_delta=add_delta, nmax=3)
    assert cut.totalphrases == 3 and cut.X.shape[1] == 1 and np.array_equal(cut.X[:, 0], ds.X[:, 0])
    assert vc.GVDataset([f.T for f in fms], add_delta=add_delta, nmax=4).X.shape[1] == 2


def test_gv_dataset_constant_row_and_large_offset(vc):
    """A row that is constant over the utterance has variance exactly 0.0 wherever the running sum of the row is exact (2.5 and
    -3e8 over 7 frames; for a value like 0.1 the computed mean is not the value, in numpy's and Julia's var as well as here, and
    the variance is ~1e-34 in all three).

    Rows 1e8 + N(0,1), T = 500, against a two-pass variance in numpy.longdouble.  The bound: a double near 1e8 is rounded at
    1e8 * eps = 2.2e-8, i.e. 2.2e-8 of the unit standard deviation.  A two-pass variance sees the offset only through the
    computed mean m: sum (x - m)^2 = sum (x - mu)^2 + T (mu - m)^2, so an error of m enters squared (naive summation:
    |mu - m| <= T u 1e8 = 5.5e-6, squared 3e-11), and x - m is exact (both within a factor 2); what is left is the
    rounding of 500 squares and adds, ~T eps = 1e-13.  1e-7 relative leaves room for a few roundings at 1e8 entering at first
    order, and nothing more: the one-pass formula sum x^2 - T m^2 cancels 1e16 against 1e16 +- 500 and loses every digit."""
    rng = np.random.default_rng(14)
    fm = rng.standard_normal((7, 4))
    fm[:, 2] = 2.5
    fm[:, 3] = -3.0e8
    X = vc.GVDataset([fm.T], ignore0th=False).X
    assert X[2, 0] == 0.0 and X[3, 0] == 0.0 and np.all(X[:2, 0] > 0)
    Xd = vc.GVDataset([fm.T], ignore0th=False, add_delta=True).X     # delta row of a constant: 2.5 at both ends, 0 between
    assert Xd[2, 0] == 0.0 and abs(Xd[6, 0] - 125 / 84) < 1e-14     # (2 (2.5 - 5/7)^2 + 5 (5/7)^2) / 6
    big = 1e8 + rng.standard_normal((500, 5))
    got = vc.GVDataset([big.T], ignore0th=False).X[:, 0]
    xl = big.astype(np.longdouble)
    ref = ((xl - xl.mean(axis=0)) ** 2).sum(axis=0) / 499
    assert np.max(np.abs(got - ref) / ref) < 1e-7


def test_gv_dataset_non_finite_values(vc):
    """src/datasets.jl:163-179: an utterance whose variance has a NaN is SKIPPED (:164), and what was kept must be finite
    (@assert, :179).  A NaN or an Inf among the frames makes the variance NaN (Inf - Inf in the deviations), so the reference
    skips that utterance, in a one-frame utterance as in a long one; the assertion is reached by a variance that overflows."""
    from oracle import np_oracle as npo
    rng = np.random.default_rng(15)
    good = [rng.standard_normal((T, 4)) for T in (9, 1, 12)]
    want = npo.gv_dataset(good).T
    for bad in (np.nan, np.inf, -np.inf):
        fms = [g.copy() for g in good]
        fms[1][0, 2] = bad                                           # in the one-frame utterance, which is skipped anyway
        assert np.array_equal(vc.GVDataset([f.T for f in fms]).X, want)
        fms[2][5, 2] = bad                                           # in a long one: its variance is NaN -> skipped as well
        ds = vc.GVDataset([f.T for f in fms])
        ref = npo.gv_dataset(fms).T
        assert ds.totalphrases == 3 and ds.X.shape == ref.shape == (3, 1) and np.array_equal(ds.X, want[:, :1])
    fms = [g.copy() for g in good]
    fms[2][5, 2], fms[2][6, 2] = 1e200, -1e200                      # finite frames, variance +Inf: kept, then the @assert
    with np.errstate(over="ignore"):
        assert np.isinf(npo.gv_dataset(fms)[1, 1])
    with pytest.raises(AssertionError):
        vc.GVDataset([f.T for f in fms])
    fms[1][0, 2] = 1e200                                             # one frame: nothing to overflow, skipped
    fms[2] = good[2]
    assert np.array_equal(vc.GVDataset([f.T for f in fms]).X, want)


def test_push_delta_and_constructW_host_helpers(vc):
    from oracle import c_oracle as co
    rng = np.random.default_rng(1)
    for T in (1, 2, 3, 17):
        s = rng.standard_normal((T, 5))
        assert np.array_equal(vc.push_delta(s.T), co.push_delta(s).T)
    import scipy.sparse as sp
    r, c, v = co.constructW(4, 6)
    ref = sp.coo_matrix((v, (r - 1, c - 1)), shape=(48, 24)).tocsc()
    assert abs(vc.constructW(4, 6) - ref).max() == 0
    assert vc.constructW(3, 1).nnz == 3


def test_dtw_online_update_and_backward_host_logic(vc):
    """update!/set_template!/backward (src/dtw.jl:53-90,133-145) are host-side in the mirror: check them against
    the oracle's fit! tables."""
    from oracle import c_oracle as co
    rng = np.random.default_rng(2)
    t = rng.standard_normal((9, 3))
    s = rng.standard_normal((7, 3))
    for fs, bs in ((0, 1), (0, 2), (1, 2)):
        p, c, b = co.dtw_fit(t, s, fs, bs)
        d = vc.DTW(fstep=fs, bstep=bs)
        vc.set_template_(d, t.T)
        assert d.costtable.shape == (9, 1) and d.costtable[:, 0].tolist() == list(range(1, 10))
        for k in range(7):
            vc.update_(d, s[k])
        assert np.array_equal(d.costtable, c.T) and np.array_equal(d.backpointer, b.T)
        assert np.array_equal(vc.backward(d), p)


def test_sharding_helpers(vc):
    from voiceconversion_jl_amd import dist as vd
    for n, world in ((10, 3), (1_000_000, 8), (5, 8), (0, 2)):
        spans = [vd.shard_range(n, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        sizes = [hi - lo for lo, hi in spans]
        assert max(sizes) - min(sizes) <= 1
    costs = [500 * 500, 100, 450 * 520, 300 * 300, 7, 550 * 550, 480 * 500]
    parts = vd.shard_by_cost(costs, 3)
    assert sorted(i for p in parts for i in p) == list(range(len(costs)))
    loads = [sum(costs[i] for i in p) for p in parts]
    assert max(loads) <= 1.5 * (sum(costs) / 3)
    S0, S1, S2 = np.arange(3.), np.arange(12.).reshape(4, 3), -np.arange(12.).reshape(4, 3)
    packed = vd.pack_stats(S0, S1, S2, 7.5)
    a0, a1, a2, ll = vc.unpack_stats(packed, 4, 3)
    assert np.array_equal(a0, S0) and np.array_equal(a1, S1) and np.array_equal(a2, S2) and ll == 7.5
    assert len(packed) == vc.stats_len(4, 3)


def test_mstep_formulas(vc):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((500, 4)) * 0.5 + 2.0
    S0 = np.array([500.0])
    S1 = X.sum(0)[:, None]
    S2 = (X * X).sum(0)[:, None]
    w, mu, var = vc.mstep_diag(S0, S1, S2, min_covar=0.0)
    assert np.allclose(w, 1.0) and np.allclose(mu[:, 0], X.mean(0)) and np.allclose(var[:, 0], X.var(0), rtol=1e-9)


def test_generated_asm_includes_match_their_generators(tmp_path):
    """csrc/dtw_fused_asm.inc and csrc/dtw_obs_asm.inc are generated files that are committed (the build has no Python
    step): regenerate both and compare byte for byte, so that neither the generator nor the file can drift alone."""
    import subprocess
    import sys
    for gen, inc in (("gen_dtw_fused_asm.py", "dtw_fused_asm.inc"), ("gen_dtw_obs_asm.py", "dtw_obs_asm.inc")):
        out = tmp_path / inc
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", gen), str(out)], check=True)
        committed = open(os.path.join(ROOT, "voiceconversion.jl_amd", "csrc", inc), "rb").read()
        assert out.read_bytes() == committed, f"{inc} differs from what tools/{gen} generates"


def test_debug_hook_is_inert_without_the_test_environment():
    """vcmi_debug_force is a process-global switch of kernel selection that the product library exports for the parity tests
    (VERDICT r2 hygiene): it must refuse unless the process was started with VCMI_TEST_HOOKS=1."""
    import subprocess
    import sys
    code = ("import ctypes, sys; lib = ctypes.CDLL(%r); lib.vcmi_debug_force.argtypes = [ctypes.c_uint]; "
            "sys.exit(0 if lib.vcmi_debug_force(32) == 0 else 3)" % os.path.join(ROOT, "voiceconversion.jl_amd", "libvcmi.so"))
    env = {k: v for k, v in os.environ.items() if k != "VCMI_TEST_HOOKS"}
    assert subprocess.run([sys.executable, "-c", code], env=env).returncode == 3
    assert subprocess.run([sys.executable, "-c", code], env=dict(env, VCMI_TEST_HOOKS="1")).returncode == 0
