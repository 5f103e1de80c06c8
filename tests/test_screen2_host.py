"""CPU: the second look of the bf16 screen, host side (csrc/gmmmap_prepare.cpp: the sixteen strongest rows per mixture and
pack_screen2_bf16; csrc/gmmmap_layout.hpp: screen2_*).  tests/c/screen2_check.cpp is a stand-alone program: it replays the look's
arithmetic from the packed image and checks, for every mixture at a few hundred points, that the certified bound is an upper
bound of the exact log-density and never above the four-row bound.  Built with ASan + UBSan like the drivers of
tests/test_sanitizers.py, so a packer that writes or reads past an image is a finding as well."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "voiceconversion.jl_amd", "csrc")
OUT = os.path.join(ROOT, "oracle", "_build")
CMD = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
       os.path.join(ROOT, "tests", "c", "screen2_check.cpp")] + [os.path.join(CSRC, f) for f in ("core.cpp", "hostpipe.cpp", "devgroup.cpp", "gmmmap_prepare.cpp")]
LINK = ["-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-ldl", "-lpthread"]


def test_second_look_image_and_bound_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "screen2_check_asan")
    subprocess.run(CMD + ["-fsanitize=address,undefined", "-o", exe] + LINK, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout)
    assert p.returncode == 0 and "screen2_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
