#!/usr/bin/env python3
"""Resource lines of every kernel in the device assembly that `hipcc --save-temps` (or `--offload-device-only -S`) leaves for a
translation unit, and, given a second file, the kernels whose lines differ between the two (either side may be several files
joined by commas, for code that moved between translation units):

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-fast-math -mllvm -amdgpu-mfma-vgpr-form --offload-device-only -S \\
        voiceconversion.jl_amd/csrc/gmmmap.hip -o gmmmap.s
    tools/kernel_resources.py parent/gmmmap.s gmmmap.s

Kernels are matched by their demangled name without the argument list, so a kernel whose signature changed still lines up.
A kernel is marked when it spills where the other build did not, gained a private segment, or needs more 8-register
allocation granules than a step of waves per SIMD allows (512 registers per lane and SIMD)."""
import re
import subprocess
import sys


def parse(paths):
    out = {}
    for path in paths.split(","):
        out.update(parse_one(path))
    return out


def parse_one(path):
    s = open(path).read()
    out = {}
    for blk in s[s.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)          # noqa: E731
        out[g("name")] = dict(vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), spill=int(g("vgpr_spill_count")),
                              lds=int(g("group_segment_fixed_size")), private=int(g("private_segment_fixed_size")))
    return out


def waves(vgpr):
    return min(8, 512 // ((vgpr + 7) // 8 * 8))


def short_names(d):
    """mangled name -> the demangled one without its argument list: a kernel whose signature changed still lines up"""
    names = sorted(d)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"\(.*", "", x).replace("void vcmi::", ""): d[n] for n, x in zip(names, dem)}


def main():
    a = short_names(parse(sys.argv[1]))
    b = short_names(parse(sys.argv[2])) if len(sys.argv) > 2 else None
    names = sorted(set(a) | set(b or {}))
    worse = 0
    for d in names:
        x, y = a.get(d), (b or {}).get(d)
        if b is None:
            print(d, x)
        elif x != y:
            bad = x and y and (waves(y["vgpr"]) < waves(x["vgpr"]) or y["spill"] > x["spill"] or y["private"] > x["private"])
            worse += bool(bad)
            print(f"{d}\n   {x}\n   {y}{'   <-- worse' if bad else ''}")
    if b is not None:
        print(f"{sum(a.get(n) != b.get(n) for n in names)} of {len(names)} kernels differ, {worse} for the worse")
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
