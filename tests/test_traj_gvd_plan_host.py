"""CPU: the launch rule of traj_gvd_kernel and the workspace arithmetic of a GV call over diagonal conditional precisions
(csrc/traj_band_plan.hpp, host arithmetic only).  tests/c/traj_gvd_plan_check.cpp is a stand-alone program that asserts the rule's
invariants for every static dimension up to 512 and prints the rule at a grid of shapes; here it is built with ASan + UBSan like
tests/test_traj_diag_host.py's, run, and its table compared with the rule as tests/gv_diag_restatement.py restates it."""
import os
import subprocess

import gv_diag_restatement as gd
from conftest import ROOT

OUT = os.path.join(ROOT, "oracle", "_build")
CMD = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "traj_gvd_plan_check.cpp")]


def test_launch_rule_under_asan_ubsan_and_against_the_restatement():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "traj_gvd_plan_check_asan")
    subprocess.run(CMD + ["-fsanitize=address,undefined", "-o", exe], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and "traj_gvd_plan_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    rows = [tuple(int(v) for v in line.split()[1:]) for line in p.stdout.splitlines() if line.startswith("rule ")]
    assert len(rows) == 9 * 25 and {r[2] for r in rows} == {0, 2, 3, 4, 5}
    for D, T, resident, lds in rows:
        assert gd.gvd_resident(D, T) == resident, (D, T)
        assert lds == (2 * gd.GVD_THREADS + 3 * D) * 8 + resident * T * D * 8 <= gd.LDS_LIMIT
