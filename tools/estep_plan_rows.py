"""One diagonal E-step per row of the plan table (tests/c/estep_plan_check.cpp) that fits in memory, and nothing else on the
device: the packed statistics of row i go to <dir>/row_<i>.npy, one summary line per row to stdout.  Frames are made on the
host and copied up, so a kernel trace of the run holds the E-step's kernels only (tools/kernel_trace_lines.py prints them;
`estep_plan_check --sequence` prints what the plan says for a row).  profiles/estep_plan/README.md: how the two are compared.
Usage: VCMI_TEST_HOOKS=1 [LIBVCMI_PROBE=other/libvcmi.so] python tools/estep_plan_rows.py <dir>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import voiceconversion_jl_amd as vc  # noqa: E402
from voiceconversion_jl_amd import _lib  # noqa: E402

A, H, S = vc.ESTEP_AUTO, vc.ESTEP_HARD, vc.ESTEP_SOFT
ROWS = [  # N, Dj, M, path, debug flags
    (1000, 80, 8, A, 0), (1000, 80, 17, A, 0), (1000, 80, 33, A, 0), (1000, 80, 65, A, 0),
    (65535, 80, 32, A, 0), (65536, 80, 32, A, 0), (65536, 80, 16, A, 0), (65536, 80, 16, H, 0), (65536, 80, 16, S, 0),
    (65536, 80, 16, A, _lib.DBG_ESTEP_NO_HARD), (1250000, 80, 128, A, 0),
    (1000, 82, 8, A, 0), (1000, 112, 8, A, 0), (1000, 114, 8, A, 0), ((1 << 20) + 1, 160, 128, A, 0),
    (1000, 81, 8, A, 0), (1000, 161, 8, A, 0), (1000, 162, 8, A, 0), (1000, 80, 129, A, 0),
    (1000, 80, 64, A, _lib.DBG_ESTEP_WAVE_KERNEL), (1000, 80, 65, A, _lib.DBG_ESTEP_WAVE_KERNEL),
    (1000, 80, 8, A, _lib.DBG_ESTEP_GENERIC), (1000, 80, 8, A, _lib.DBG_ESTEP_NO_SMALL), (1000, 80, 17, A, _lib.DBG_ESTEP_NO_SMALL),
]


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    for i, (N, Dj, M, path, flags) in enumerate(ROWS):
        rg = np.random.default_rng(1000 + i)
        w = rg.dirichlet(2.0 * np.ones(M))
        var = np.exp(rg.uniform(np.log(0.05), 0.0, (M, Dj)))
        mu = 3.0 * rg.standard_normal((M, Dj))
        comp = rg.choice(M, size=N, p=w)
        X = rg.standard_normal((N, Dj), dtype=np.float32).astype(np.float64)
        X *= np.sqrt(var[comp])
        X += mu[comp]
        Xd = torch.from_numpy(X).cuda()
        torch.cuda.synchronize()
        vc.estep_set_path(path)
        _lib.debug_force(flags)
        try:
            stats = vc.estep_diag_dev(Xd.t(), w, mu.T, var.T)
            torch.cuda.synchronize()
            soft = _lib.estep_last_soft()
        finally:
            _lib.debug_force(0)
            vc.estep_set_path(A)
        h = stats.cpu().numpy()
        np.save(os.path.join(out, "row_%02d.npy" % i), h)
        print("row %02d N=%d Dj=%d M=%d path=%d flags=%d soft=%d S0sum=%.6f ll=%.9e" % (i, N, Dj, M, path, flags, soft, h[:M].sum(), h[-1]), flush=True)
        del Xd, stats


if __name__ == "__main__":
    main()
