"""CPU: the host planning of the fused DTW path (csrc/dtw_plan.cpp: pair order and workspace offsets, row strips, packed groups,
column segments, job order and the flags between jobs).  tests/c/dtw_plan_check.cpp is a stand-alone program that asserts exact
facts on 144 plans -- above all that a job waits only on flags signalled by a strictly earlier job, on which the persistent
forward kernel's freedom from deadlock rests -- and compares three small plans with hand-written descriptors, so it needs no
tolerance and no device.  Built with ASan + UBSan like tests/test_vc_batch_host.py; nothing is loaded into Python."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "voiceconversion.jl_amd", "csrc")
OUT = os.path.join(ROOT, "oracle", "_build")
CMD = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "dtw_plan_check.cpp"),
       os.path.join(CSRC, "dtw_plan.cpp")]


def test_dtw_fused_plan_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "dtw_plan_check_asan")
    subprocess.run(CMD + ["-fsanitize=address,undefined", "-o", exe], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout)
    assert p.returncode == 0 and "dtw_plan_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]

