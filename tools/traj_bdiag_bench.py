"""BlockDiagTrajectoryGMMMap (trajectory conversion straight from a cross-diagonal model: vcmi_traj_create_bdiag) against the
detour through the expanded model, TrajectoryGMMMap(GMMMap(w, mu, expand_block_diag(covars)), T, precision="diag"),
device-resident.

  shape:   M = 64, 256 utterances x 2000 frames, static D = 40 and D = 59 (tools/traj_diag_bench.py's), one cross-diagonal model
           per dimension (Dj = 4D), frames a scaled cumulative sum of draws from it with their deltas
  timing:  HIP events around vcmi_traj_convert_batch_dev after warm-up calls; the calls of the two paths ALTERNATE in one
           process, so clock drift lands on both; per path every time, the median and the spread (max - min) / median
  build:   host time of constructing each converter from the same (w, mu, covars), time.perf_counter around the constructors
           (the detour expands the covariances and inverts M dense blocks), the median of three
  kernels: with --kernels every (dimension, path) runs once more in a child process under `rocprofv3 --kernel-trace --stats`
           (tracing only: no counters), and the per-kernel average durations of that child's calls are added -- the split of the
           call between the arg-max / g_t stage and the solver.  For the fused pass (bdmap_kernel<3, .>) its share of two roofs:
           FP64 vector -- per frame and mixture 2D (subtract, multiply, fma) = 3 operations of the log-density, plus 2D x 3 of
           g_t, as 2 flop each over --peak-tflops (78.6: MI355X vector FP64) -- and HBM: the x read and the g store of 2D doubles
           each and the 8-byte index per frame over --peak-tbs (8.0)

Usage: python tools/traj_bdiag_bench.py [--dims 40,59] [--utts 256] [--frames 2000] [--reps 7] [--kernels] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M = 64
PATHS = ("bdiag", "detour")


def median(v):
    return float(np.median(np.asarray(v)))


def model(D):
    """w (M,), mu (4D,M), covars (6D,M): variances log-uniform in [0.05, 1] per dimension, pair correlations uniform in
    (-0.9, 0.9), both varied a little per mixture; means 0.7 / sqrt(4D) N(0,1), so that neighbouring mixtures share frames"""
    rng = np.random.default_rng(1005 + D)
    Dj, D2 = 4 * D, 2 * D
    w = rng.dirichlet(4.0 * np.ones(M))
    mu = np.asfortranarray(0.7 / np.sqrt(Dj) * rng.standard_normal((Dj, M)))
    var = np.exp(rng.uniform(np.log(0.05), 0.0, (Dj, 1)) + 0.7 / np.sqrt(Dj) * rng.standard_normal((Dj, M)))
    rho = np.clip(rng.uniform(-0.9, 0.9, (D2, 1)) + 0.3 / np.sqrt(D2) * rng.standard_normal((D2, M)), -0.9, 0.9)
    return w, mu, np.asfortranarray(np.vstack([var, rho * np.sqrt(var[:D2] * var[D2:])]))


def frames(vc, rng, w, mu, cov, T, D):
    """(T,2D): source-static draws of the model, cumulative sum scaled by 1/sqrt(t), with their deltas"""
    comp = rng.choice(M, size=T, p=w)
    st = mu[:D].T[comp] + np.sqrt(cov[:D]).T[comp] * rng.standard_normal((T, D))
    st = np.cumsum(st, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
    return np.ascontiguousarray(vc.push_delta(np.asfortranarray(st.T)).T)


def build(vc, path, w, mu, cov, T):
    if path == "bdiag":
        return vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(w, mu, cov), T)
    return vc.TrajectoryGMMMap(vc.GMMMap(w, mu, vc.expand_block_diag(cov)), T, precision="diag")


def measure(vc, lib, torch, D, n, T, reps, warmup, paths=PATHS):
    w, mu, cov = model(D)
    conv, build_ms = {}, {}
    for p in paths:
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            conv[p] = build(vc, p, w, mu, cov, T)
            ts.append((time.perf_counter() - t0) * 1e3)
        build_ms[p] = ts
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
    last = {}
    for _ in range(reps):
        for p in paths:
            times[p].append(call(p))
            if p not in last:
                last[p] = Yd.clone()
    assert all(bool(torch.isfinite(y).all()) for y in last.values())
    res = {"D": D, "utterances": n, "frames_per_utterance": T, "reps": reps}
    for p in paths:
        md = median(times[p])
        res[p] = {"call_ms": times[p], "call_median_ms": md, "call_spread": (max(times[p]) - min(times[p])) / md,
                  "frames_per_s": n * T / (md * 1e-3), "build_ms": build_ms[p], "build_median_ms": median(build_ms[p])}
    if len(paths) == 2:
        a, b = res["bdiag"], res["detour"]
        res["detour_over_bdiag"] = b["call_median_ms"] / a["call_median_ms"]
        # faster by more than the two spreads combined
        res["gain_ms"] = b["call_median_ms"] - a["call_median_ms"]
        res["spreads_combined_ms"] = a["call_spread"] * a["call_median_ms"] + b["call_spread"] * b["call_median_ms"]
        res["max_rel_difference_of_the_two_results"] = float((last["bdiag"] - last["detour"]).abs().max() / last["detour"].abs().max())
    return res


def kernel_split(D, path, n, T, reps):
    """per-kernel average durations (us) and calls of `reps` + 1 calls of one path, traced in a child process"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--", sys.executable,
               os.path.abspath(__file__), "--dims", str(D), "--only", path, "--utts", str(n), "--frames", str(T), "--reps", str(reps),
               "--warmup", "1"]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=d, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return {"error": (p.stderr or p.stdout)[-400:]}
        rows = list(csv.DictReader(open(files[0])))
    return {r["Name"].split("(")[0][-60:]: {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "percent": float(r["Percentage"])}
            for r in rows[:8]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="40,59")
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--only", default=None, choices=PATHS, help="one path only (the traced child of --kernels)")
    ap.add_argument("--kernels", action="store_true", help="add the per-kernel split from a traced child process per (dimension, path)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import _lib
    import bench
    assert torch.cuda.is_available(), "traj_bdiag_bench needs a HIP device (there is no CPU fallback)"
    dims = [int(d) for d in a.dims.split(",")]
    paths = (a.only,) if a.only else PATHS
    out = {"tool": "traj_bdiag_bench", "M": M, "device": torch.cuda.get_device_name(0), "source_hash": bench.source_hash(),
           "args": {k: v for k, v in vars(a).items() if k != "out"},
           "results": [measure(vc, _lib, torch, D, a.utts, a.frames, a.reps, a.warmup, paths) for D in dims]}
    if a.kernels:
        for r in out["results"]:
            for p in paths:
                r[p]["kernels"] = ks = kernel_split(r["D"], p, a.utts, a.frames, min(a.reps, 3))
                fused = [v for k, v in ks.items() if "bdmap_kernel" in k and isinstance(v, dict)]
                if p == "bdiag" and fused:
                    D2, N, t = 2 * r["D"], r["utterances"] * r["frames_per_utterance"], fused[0]["avg_us"] * 1e-6
                    r[p]["fused_pass_us"] = fused[0]["avg_us"]
                    r[p]["fused_fp64_vector_roof_fraction"] = 2.0 * 3 * D2 * (M + 1) * N / t / (a.peak_tflops * 1e12)
                    r[p]["fused_hbm_roof_fraction"] = (16.0 * D2 + 8.0) * N / t / (a.peak_tbs * 1e12)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
