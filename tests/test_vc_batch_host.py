"""CPU: the host planning of vc_batch (csrc/vc_batch_plan.cpp: the refusal verdicts, the chunk list, the work lists of the three
segmented kernels and the offsets).  tests/c/vc_batch_plan_check.cpp is a stand-alone program that asserts exact facts at
T = [0, 1, 2, L-1, L, L+1, 2L+1, 2048, 2049] and L in {1, 20}, so it needs no tolerance and no device.  Built with ASan + UBSan
like tests/test_traj_prepare_host.py; nothing is loaded into Python."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "voiceconversion.jl_amd", "csrc")
OUT = os.path.join(ROOT, "oracle", "_build")
CMD = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "vc_batch_plan_check.cpp"),
       os.path.join(CSRC, "vc_batch_plan.cpp")]


def test_vc_batch_plan_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "vc_batch_plan_check_asan")
    subprocess.run(CMD + ["-fsanitize=address,undefined", "-o", exe], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout)
    assert p.returncode == 0 and "vc_batch_plan_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


def test_the_binding_reaches_every_batch_entry():
    """the five C entries are declared, exported and bound; the Julia module calls the three host-pointer ones"""
    from voiceconversion_jl_amd import _lib
    import voiceconversion_jl_amd as vc
    new = ("vcmi_vc_frames_batch", "vcmi_vc_traj_batch", "vcmi_vc_trajgv_batch", "vcmi_vc_traj_batch_dev", "vcmi_vc_trajgv_batch_dev")
    header = open(os.path.join(ROOT, "include", "vcmi.h")).read()
    jl = open(os.path.join(ROOT, "voiceconversion.jl_amd", "julia", "VoiceConversionMI.jl")).read()
    for sym in new:
        assert sym in _lib.SIGNATURES and hasattr(_lib.lib, sym) and f"int {sym}(" in header
    for sym in new[:3]:
        assert f"(:{sym}, libvcmi)" in jl, sym
    assert callable(vc.vc_batch)
