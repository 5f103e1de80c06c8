"""Frame-by-frame conversion with a cross-diagonal model, at D = 40, M = 64 on 1e6 frames and D = 80, M = 64 on 5e5 frames, two
routes on the SAME device-resident frames:

  bdiag_*     BlockDiagGMMMap (vcmi_bdmap_*, csrc/gmmmap_bdiag.hip), the model as trained;
  expanded_*  GMMMap on expand_block_diag(covars): the only route without it (the dense MFMA convert kernel).

fvconvert and predict of each.  Models from tests/em_bdiag_restatement.bdiag_model, frames from its draw (the source half).
Each figure is the median over R repetitions of K calls timed with HIP events (after W warm-up calls), the contenders
alternating; the spread (max - min) / median is reported with it.  roof fractions of bdiag fvconvert: the FP64 vector
operations the kernel issues per frame, 6 D M (3 for the centred log-density, 3 for the centred regression and its
accumulation), as 2 flop each over the time and the FP64 peak (--peak-tflops, 78.6: MI355X vector FP64), and the 16 D bytes per
frame over the time and the HBM peak (--peak-tbs, 6.3).  --only expanded runs on a tree without the new converter (the parent
commit).  Prints one JSON line.
Usage: python tools/gmmmap_bdiag_bench.py [--shapes 40:64:1000000,80:64:500000] [--warmup W] [--steps K] [--reps R] [--only a,b]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def expand(cov):
    D, M = cov.shape[0] // 3, cov.shape[1]
    out = np.zeros((2 * D, 2 * D, M), order="F")
    for m in range(M):
        out[:, :, m] = np.diag(cov[:2 * D, m]) + np.diag(cov[2 * D:, m], D) + np.diag(cov[2 * D:, m], -D)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="40:64:1000000,80:64:500000")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="bdiag,expanded")
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    ap.add_argument("--peak-tbs", type=float, default=6.3)
    a = ap.parse_args()
    import torch

    import em_bdiag_restatement as eb
    import voiceconversion_jl_amd as vc
    assert torch.cuda.is_available(), "gmmmap_bdiag_bench needs a HIP device (there is no CPU fallback)"
    kinds = a.only.split(",")
    out = {"tool": "gmmmap_bdiag_bench", "warmup": a.warmup, "steps": a.steps, "reps": a.reps, "results": []}
    for D, M, N in (tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")):
        w, mu, cov = eb.bdiag_model(9000 + D + M, 2 * D, M)
        X = torch.from_numpy(np.ascontiguousarray(eb.draw(9001 + N, w, mu, cov, N)[:, :D])).cuda().t()
        Y = torch.empty((N, D), dtype=torch.float64, device="cuda").t()
        conv = {}
        if "bdiag" in kinds:
            conv["bdiag"] = vc.BlockDiagGMMMap(w, mu, cov)
        if "expanded" in kinds:
            conv["expanded"] = vc.GMMMap(w, mu, expand(cov))
        jobs = {}
        for k, g in conv.items():
            jobs[k + "_fvconvert"] = (lambda g=g: vc.fvconvert(g, X, out=Y))
            jobs[k + "_predict"] = (lambda g=g: vc.predict(g.px, X))
        times = {k: [] for k in jobs}
        for fn in jobs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):                       # the contenders alternate: drift of the machine reaches all of them
            for k, fn in jobs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.steps)
        r = {"D": D, "M": M, "frames": N}
        for k, ms in times.items():
            r[k + "_ms"] = float(np.median(ms))
            r[k + "_spread"] = float((max(ms) - min(ms)) / np.median(ms))
        if "bdiag" in kinds:
            t = r["bdiag_fvconvert_ms"] * 1e-3
            r["bdiag_fp64_vector_roof_fraction"] = 2.0 * 6 * D * M * N / t / (a.peak_tflops * 1e12)
            r["bdiag_hbm_roof_fraction"] = 16.0 * D * N / t / (a.peak_tbs * 1e12)
            if "expanded" in kinds:
                for what in ("fvconvert", "predict"):
                    r[f"expanded_over_bdiag_{what}"] = r[f"expanded_{what}_ms"] / r[f"bdiag_{what}_ms"]
        out["results"].append(r)
        del X, Y, conv, jobs
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
