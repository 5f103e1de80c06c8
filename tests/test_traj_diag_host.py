"""CPU: the host arithmetic of the diagonal model of a TrajectoryGMMMap (traj_prepare_diag in csrc/traj_prepare.cpp, behind
vcmi_traj_set_precision: q_m = 1 ./ diag(Syy_m - A_m Sxy_m) and the images of diag(q_m) the g_t kernels read).
tests/c/traj_diag_prepare_check.cpp is a stand-alone program that asserts exact facts at static D = 3, 12 and 47 and the refusal of
a conditional variance that is zero, negative, NaN or infinite, so it needs no device.  Built with ASan + UBSan like
tests/test_traj_prepare_host.py."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "voiceconversion.jl_amd", "csrc")
OUT = os.path.join(ROOT, "oracle", "_build")
CMD = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
       os.path.join(ROOT, "tests", "c", "traj_diag_prepare_check.cpp")] + [os.path.join(CSRC, f) for f in ("core.cpp", "traj_prepare.cpp")]
LINK = ["-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-ldl", "-lpthread"]


def test_diagonal_model_images_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "traj_diag_prepare_check_asan")
    subprocess.run(CMD + ["-fsanitize=address,undefined", "-o", exe] + LINK, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout)
    assert p.returncode == 0 and "traj_diag_prepare_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
