"""BlockDiagTrajectoryEMGMMMap (EM re-estimation over all mixtures straight from a cross-diagonal model: vcmi_traj_set_em_bdiag)
against the detour through the expanded model, TrajectoryGMMMap(GMMMap(w, mu, expand_block_diag(covars)), T, em_iters=n),
device-resident.

  shapes:  M = 64, static D = 40 and D = 59, 256 utterances x 2000 frames and 5120 x 100 frames (vc's chunks), n = 2 iterations;
           model and frames are tools/traj_bdiag_bench.py's
  timing:  HIP events around vcmi_traj_convert_batch_dev after warm-up calls; the calls of the paths ALTERNATE in one process, so
           clock drift lands on all of them; per path every time, the median and the spread (max - min) / median.  "plain" is the
           same cross-diagonal handle with em_iters = 0: what the two iterations add to a call
  kernels: with --kernels every (shape, path) runs once more in a child process under `rocprofv3 --kernel-trace --stats` (tracing
           only: no counters), and the per-kernel average durations of that child's calls are added -- the split of an iteration
           between the fused pass, the sum and the solve.  For the fused pass (traj_em_bd_kernel<0, .>) its share of two roofs:
           FP64 vector -- 13 x 2D x M operations per frame (8 in the density phase: 3 for the source term, 5 for the target term;
           5 in the accumulation phase) as 2 flop each over --peak-tflops (78.6: MI355X vector FP64) -- and HBM: x (2D doubles)
           and y (D) read, qbar and gbar (2D each) and lse written per frame over --peak-tbs (8.0)

Usage: python tools/traj_em_bdiag_bench.py [--dims 40,59] [--shapes 256x2000,5120x100] [--iters 2] [--reps 7] [--kernels] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from traj_bdiag_bench import M, frames, median, model      # noqa: E402

PATHS = ("bdiag_em", "plain", "detour_em")


def build(vc, path, w, mu, cov, T, iters):
    if path == "bdiag_em":
        return vc.BlockDiagTrajectoryEMGMMMap(vc.BlockDiagGMMMap(w, mu, cov), T, em_iters=iters)
    if path == "plain":
        return vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(w, mu, cov), T)
    return vc.TrajectoryGMMMap(vc.GMMMap(w, mu, vc.expand_block_diag(cov)), T, em_iters=iters)


def measure(vc, lib, torch, D, n, T, iters, reps, warmup, paths):
    w, mu, cov = model(D)
    conv = {p: build(vc, p, w, mu, cov, T, iters) for p in paths}
    rng = np.random.default_rng(1005)
    base = [frames(vc, rng, w, mu, cov, T, D) for _ in range(min(n, 8))]
    Xd = torch.from_numpy(np.concatenate([base[i % len(base)] for i in range(n)])).cuda()
    Yd = torch.empty((n * T, D), dtype=torch.float64, device="cuda")
    xoff = np.arange(n, dtype=np.int64) * T * 2 * D
    yoff = np.arange(n, dtype=np.int64) * T * D
    Ts = np.full(n, T, dtype=np.int64)
    stream = torch.cuda.current_stream().cuda_stream

    def call(p):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.check(lib.lib.vcmi_traj_convert_batch_dev(conv[p]._h, n, Xd.data_ptr(), lib.iptr(xoff), lib.iptr(Ts), Yd.data_ptr(),
                                                      lib.iptr(yoff), stream))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        for p in paths:
            call(p)
    times = {p: [] for p in paths}
    last, hist = {}, {}
    for _ in range(reps):
        for p in paths:
            times[p].append(call(p))
            if p not in last:
                last[p] = Yd.clone()
                hist[p] = [float(v) for v in conv[p].em_history()]
    assert all(bool(torch.isfinite(y).all()) for y in last.values())
    res = {"D": D, "utterances": n, "frames_per_utterance": T, "iters": iters, "reps": reps}
    for p in paths:
        md = median(times[p])
        res[p] = {"call_ms": times[p], "call_median_ms": md, "call_spread": (max(times[p]) - min(times[p])) / md,
                  "frames_per_s": n * T / (md * 1e-3), "em_history": hist[p]}
    if "bdiag_em" in res and "detour_em" in res:
        a, b = res["bdiag_em"], res["detour_em"]
        res["detour_over_bdiag"] = b["call_median_ms"] / a["call_median_ms"]
        res["gain_ms"] = b["call_median_ms"] - a["call_median_ms"]
        res["spreads_combined_ms"] = a["call_spread"] * a["call_median_ms"] + b["call_spread"] * b["call_median_ms"]
        res["max_rel_difference_of_the_two_results"] = float((last["bdiag_em"] - last["detour_em"]).abs().max() / last["detour_em"].abs().max())
    if "bdiag_em" in res and "plain" in res:
        res["ms_per_iteration_over_plain"] = (res["bdiag_em"]["call_median_ms"] - res["plain"]["call_median_ms"]) / max(iters, 1)
    return res


def kernel_split(D, path, n, T, iters, reps):
    """per-kernel average durations (us) and calls of `reps` + 1 calls of one path, traced in a child process"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--", sys.executable,
               os.path.abspath(__file__), "--dims", str(D), "--only", path, "--shapes", f"{n}x{T}", "--iters", str(iters), "--reps", str(reps),
               "--warmup", "1"]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=d, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return {"error": (p.stderr or p.stdout)[-400:]}
        rows = list(csv.DictReader(open(files[0])))
    return {r["Name"].split("(")[0][-60:]: {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "percent": float(r["Percentage"])}
            for r in rows[:10]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="40,59")
    ap.add_argument("--shapes", default="256x2000,5120x100", help="utterances x frames, comma-separated")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--only", default=None, choices=PATHS, help="one path only (the traced child of --kernels)")
    ap.add_argument("--skip", default="", help="paths to leave out, comma-separated")
    ap.add_argument("--kernels", action="store_true", help="add the per-kernel split from a traced child process per (shape, path)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import _lib
    import bench
    assert torch.cuda.is_available(), "traj_em_bdiag_bench needs a HIP device (there is no CPU fallback)"
    dims = [int(d) for d in a.dims.split(",")]
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    paths = (a.only,) if a.only else tuple(p for p in PATHS if p not in a.skip.split(","))
    out = {"tool": "traj_em_bdiag_bench", "M": M, "device": torch.cuda.get_device_name(0), "source_hash": bench.source_hash(),
           "args": {k: v for k, v in vars(a).items() if k != "out"},
           "results": [measure(vc, _lib, torch, D, n, T, a.iters, a.reps, a.warmup, paths) for D in dims for n, T in shapes]}
    if a.kernels:
        for r in out["results"]:
            for p in paths:
                if p == "plain":
                    continue
                r[p]["kernels"] = ks = kernel_split(r["D"], p, r["utterances"], r["frames_per_utterance"], a.iters, min(a.reps, 3))
                fused = [v for k, v in ks.items() if "traj_em_bd_kernel" in k and isinstance(v, dict)]
                if p == "bdiag_em" and fused:
                    D2, N, t = 2 * r["D"], r["utterances"] * r["frames_per_utterance"], fused[0]["avg_us"] * 1e-6
                    r[p]["fused_pass_us"] = fused[0]["avg_us"]
                    r[p]["fused_fp64_vector_roof_fraction"] = 2.0 * 13 * D2 * M * N / t / (a.peak_tflops * 1e12)
                    r[p]["fused_hbm_roof_fraction"] = (8.0 * (3 * D2 + r["D"]) + 8.0) * N / t / (a.peak_tbs * 1e12)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
