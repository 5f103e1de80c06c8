"""CPU: the cross-diagonal frame-by-frame converter without a device.
  1. tests/gmmmap_bdiag_restatement.py (the reference and the bounds the GPU test uses) agrees with oracle/np_oracle.GMMMap on
     the expanded model, both swaps, at the shapes of the GPU parity test; the uncorrected expanded log-density misses the
     posterior bound on the cancellation case, the centred float64 one holds it (so the bound tells the two apart).
  2. Every argument error of BlockDiagGMMMap is raised before a device is touched.
  3. tests/c/gmmmap_bdiag_prepare_check.cpp: csrc/gmmmap_bdiag_prepare.cpp under ASan + UBSan, a stand-alone program built with
     the host compiler like tests/test_vc_batch_host.py; nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, frame_relerr
import em_bdiag_restatement as eb
import gmmmap_bdiag_restatement as rs

CSRC = os.path.join(ROOT, "voiceconversion.jl_amd", "csrc")
OUT = os.path.join(ROOT, "oracle", "_build")
CMD = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "gmmmap_bdiag_prepare_check.cpp"),
       os.path.join(CSRC, "gmmmap_bdiag_prepare.cpp")]


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("D,M,T", rs.PARITY_SHAPES)
def test_restatement_agrees_with_the_numpy_oracle(D, M, T, swap):
    from oracle import np_oracle as npo
    w, mu, cov = eb.bdiag_model(9000 + D + M, 2 * D, M)
    Z = eb.draw(9001 + T, w, mu, cov, T)
    X = Z[:, D:] if swap else Z[:, :D]
    X = X[::16] if T > 1000 else X          # (the oracle is a Python loop per frame and mixture: every 16th frame of the long call)
    g = npo.GMMMap(w, mu.T, np.transpose(eb.expand(cov), (2, 1, 0)), swap=swap)
    Y, P, L = rs.convert(X, w, mu, cov, swap)
    ey, ep = frame_relerr(Y.T, g.fvconvert(X).T), float(np.max(np.abs(P - g.predict_proba(X))))
    print(f"D={D} M={M} T={len(X)} swap={swap}: frame-relative {ey:.2e}, posterior {ep:.2e}")
    assert ey < 1e-13 and ep < 1e-13
    assert np.array_equal(rs.predict(L), g.predict(X))
    Yl, Pl, _ = rs.convert(X, w, mu, cov, swap, rs.LD)
    assert frame_relerr(Y.T, np.asarray(Yl, dtype=np.float64).T) < 1e-13 and np.max(np.abs(P - Pl)) < 1e-13


def test_the_bounds_separate_the_centred_from_the_expanded_form():
    w, mu, cov, Z = rs.cancellation_case()
    X = Z[:, :8]
    Yl, Pl, Ll = rs.convert(X, w, mu, cov, False, rs.LD)
    Y, P, L = rs.convert(X, w, mu, cov)
    B, PB, YB = rs.logdens_bound(X, w, mu, cov), rs.posterior_bound(X, w, mu, cov), rs.convert_bound(X, w, mu, cov)
    fl = float(np.max(np.abs(L - Ll) / B))
    fp = float(np.max(np.max(np.abs(P - Pl), axis=1) / PB))
    fy = float(np.max(np.abs(Y - Yl) / YB))
    fx = float(np.max(np.max(np.abs(rs.expanded_posterior(X, w, mu, cov) - Pl), axis=1) / PB))
    shared = float(np.mean(1.0 - np.max(np.asarray(Pl, dtype=np.float64), axis=1)))
    print(f"centred float64: {fl:.3f} of B, {fp:.4f} of the posterior bound, {fy:.4f} of the y bound; expanded form: {fx:.3g} of the "
          f"posterior bound; shared posterior mass {shared:.2f}")
    assert fl <= 1.0 and fp <= 1.0 and fy <= 1.0
    assert fx > 100.0, "the cancellation case no longer tells the expanded form apart"
    assert shared > 0.1


def test_argument_errors_need_no_device():
    import voiceconversion_jl_amd as vc
    w, mu, cov = eb.bdiag_model(1, 8, 3)
    bad = [(w, mu, cov[:-1]),                      # covars not (Dj + Dj/2, M)
           (w, mu, eb.expand(cov)),                # the expanded tensor
           (w, mu[:-1], cov),                      # odd Dj
           (w[:-1], mu, cov),                      # weights against mu
           (w, mu, cov[:, :-1]),                   # covars against mu
           (np.ones(2) / 2, np.zeros((258, 2)), np.ones((387, 2))),       # D = 129
           (np.ones(257) / 257, np.zeros((4, 257)), np.ones((6, 257)))]   # M = 257
    for args in bad:
        with pytest.raises((vc.DimensionMismatch, ValueError)) as e:
            vc.BlockDiagGMMMap(*args)
        if np.ndim(args[2]) == 2:
            assert isinstance(e.value, vc.DimensionMismatch), e.value
    assert issubclass(vc.BlockDiagGMMMap, vc.FrameByFrameConverter)


def test_prepare_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "gmmmap_bdiag_prepare_check_asan")
    subprocess.run(CMD + ["-fsanitize=address,undefined", "-o", exe], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout)
    assert p.returncode == 0 and "gmmmap_bdiag_prepare_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
