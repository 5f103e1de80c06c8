"""CPU: the launch plan of the diagonal E-step (csrc/estep_plan.cpp: route, body, hard-assignment chain, every grid, the rows of
every reduction, every scratch reservation).  tests/c/estep_plan_check.cpp is a stand-alone program that compares hand-derived
plans -- one per route, body and decision boundary -- field by field and asserts bounds over a sweep of shapes (partial rows
fit their buffer, the sample lies inside the chunks, the sort scratch and the piece count hold any assignment of frames), so it
needs no tolerance and no device.  Built with ASan + UBSan like tests/test_dtw_plan_host.py; nothing is loaded into Python."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "voiceconversion.jl_amd", "csrc")
OUT = os.path.join(ROOT, "oracle", "_build")
CMD = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "estep_plan_check.cpp"),
       os.path.join(CSRC, "estep_plan.cpp")]


def test_estep_plan_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "estep_plan_check_asan")
    subprocess.run(CMD + ["-fsanitize=address,undefined", "-o", exe], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout)
    assert p.returncode == 0 and "estep_plan_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
