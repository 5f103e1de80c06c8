"""CPU: trajectory conversion straight from a cross-diagonal model, without a device.
  1. tests/c/traj_bdiag_prepare_check.cpp: what csrc/gmmmap_bdiag_prepare.cpp makes for vcmi_traj_create_bdiag -- q and the
     [mu_x, a, mu_y, q] table bit for bit against the plain expressions at (Dj, M) = (4, 1), (12, 3), (256, 2) with and without
     swap, zero padding rows, the index of a valid pair whose conditional variance rounds to <= 0, and the frame-by-frame tables
     unchanged by the extension -- a stand-alone program under ASan + UBSan, built like tests/test_traj_diag_host.py builds its
     check; nothing is loaded into Python.
  2. The argument errors of BlockDiagTrajectoryGMMMap that are raised before a device is touched, and the package's export."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "voiceconversion.jl_amd", "csrc")
OUT = os.path.join(ROOT, "oracle", "_build")
CMD = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "traj_bdiag_prepare_check.cpp"),
       os.path.join(CSRC, "gmmmap_bdiag_prepare.cpp")]


def test_trajectory_tables_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "traj_bdiag_prepare_check_asan")
    subprocess.run(CMD + ["-fsanitize=address,undefined", "-o", exe], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout)
    assert p.returncode == 0 and "traj_bdiag_prepare_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


def test_constructor_takes_a_block_diag_gmmmap_only():
    import voiceconversion_jl_amd as vc
    assert issubclass(vc.BlockDiagTrajectoryGMMMap, vc.TrajectoryGMMMap)
    for g in (None, object(), "model", 3):
        with pytest.raises(TypeError, match="BlockDiagGMMMap"):
            vc.BlockDiagTrajectoryGMMMap(g, 10)
