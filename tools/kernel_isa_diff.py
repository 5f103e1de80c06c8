#!/usr/bin/env python3
"""Instruction streams of the kernels in gfx950 code objects, compared symbol by symbol between two sets of files:

    tools/kernel_isa_diff.py parent/traj.co -- traj.co traj_solve.co traj_gv.co traj_em.co [--match traj_]

Each file is disassembled with the ROCm llvm-objdump -d (branch targets are relative there, and labels carry no function
numbers); the address column is dropped, the instruction text and its encoding are kept.  Trailing s_code_end / s_nop lines of
every symbol are dropped: the assembler pads behind the last function of a file, and nothing executes behind a kernel's end.  Prints every symbol that is missing on
one side or whose stream differs, then "N of N kernels identical"; exit status 1 unless all are."""
import re
import subprocess
import sys

OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"


def streams(paths, match):
    out = {}
    for path in paths:
        text = subprocess.run([OBJDUMP, "-d", path], capture_output=True, text=True, check=True).stdout
        sym = None
        for line in text.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                sym = m.group(1) if match in m.group(1) else None
                if sym:
                    out[sym] = []
            elif sym and line.startswith("\t"):
                out[sym].append(re.sub(r"// [0-9A-Fa-f]+:", "//", line))
    for ins in out.values():       # padding behind the end of a function belongs to no kernel
        while ins and re.match(r"\s*(s_code_end|s_nop)\b", ins[-1]):
            ins.pop()
    return out


def main():
    args = sys.argv[1:]
    match = "traj_"
    if "--match" in args:
        i = args.index("--match")
        match = args[i + 1]
        del args[i:i + 2]
    i = args.index("--")
    a, b = streams(args[:i], match), streams(args[i + 1:], match)
    names = sorted(set(a) | set(b))
    same = 0
    for n in names:
        if n not in a or n not in b:
            print("only in the", "first" if n in a else "second", "set:", n)
        elif a[n] != b[n]:
            k = next((j for j, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
            print(f"differs: {n}: {len(a[n])} / {len(b[n])} instructions, first difference at {k}")
        else:
            same += 1
    print(f"{same} of {len(names)} kernels identical")
    return 0 if same == len(names) else 1


if __name__ == "__main__":
    sys.exit(main())
