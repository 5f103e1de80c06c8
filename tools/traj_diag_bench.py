"""TrajectoryGMMMap with full and with diagonal conditional precisions (vcmi_traj_set_precision), device-resident.

  shape:   M = 64, 256 utterances x 2000 frames, static D = 40 and D = 59 -- bench.py's `traj` workload and the widest cepstra the
           pipeline takes -- through vcmi_traj_convert_batch_dev, in both modes on ONE handle
  timing:  HIP events around the entry after warm-up calls; the calls of the two modes ALTERNATE, so clock drift lands on both
  kernels: with --kernels every (dimension, mode) runs once more in a child process under `rocprofv3 --kernel-trace --stats`
           (tracing only: no counters), and the per-kernel average durations of that child's calls are added -- the split of the
           call between arg-max, g_t and the solver

Per (dimension, mode) the JSON line holds every time, the median, the spread of the repeats ((max - min) / median) and frames/s;
per dimension the ratio of the two medians and the largest difference between the two results (they are different models: a
magnitude, not a check).
Usage: python tools/traj_diag_bench.py [--dims 40,59] [--utts 256] [--frames 2000] [--reps 7] [--kernels] [--out FILE]"""
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
import synthdata as sd  # noqa: E402

M = 64
MODES = ("full", "diag")


def median(v):
    return float(np.median(np.asarray(v)))


def setup(vc, torch, D, n, T):
    w, mu, sig = sd.synth_model(1005 + D, 4 * D, M, lam_lo=1e-3)
    g = vc.GMMMap(w, np.asfortranarray(mu.T), np.asfortranarray(np.transpose(sig, (2, 1, 0))))
    tj = vc.TrajectoryGMMMap(g, T)
    rng = np.random.default_rng(1005)
    base = []
    for _ in range(min(n, 8)):
        st = sd.sample_frames(int(rng.integers(1 << 30)), w, mu, sig, T, 0, D)
        st = np.cumsum(st, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
        base.append(np.ascontiguousarray(vc.push_delta(np.asfortranarray(st.T)).T))       # (T,2D)
    Xd = torch.from_numpy(np.concatenate([base[i % len(base)] for i in range(n)])).cuda()
    Yd = torch.empty((n * T, D), dtype=torch.float64, device="cuda")
    xoff = np.arange(n, dtype=np.int64) * T * 2 * D
    yoff = np.arange(n, dtype=np.int64) * T * D
    Ts = np.full(n, T, dtype=np.int64)
    return g, tj, Xd, Yd, xoff, yoff, Ts


def measure(vc, lib, torch, D, n, T, reps, warmup, modes=MODES):
    g, tj, Xd, Yd, xoff, yoff, Ts = setup(vc, torch, D, n, T)
    stream = torch.cuda.current_stream().cuda_stream

    def call(mode):
        tj.precision = mode
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.check(lib.lib.vcmi_traj_convert_batch_dev(tj._h, n, Xd.data_ptr(), lib.iptr(xoff), lib.iptr(Ts), Yd.data_ptr(),
                                                      lib.iptr(yoff), stream))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        for m in modes:
            call(m)
    times = {m: [] for m in modes}
    last = {}
    for _ in range(reps):
        for m in modes:
            times[m].append(call(m))
            if m not in last:
                last[m] = Yd.clone()
    assert all(bool(torch.isfinite(y).all()) for y in last.values())
    frames = n * T
    res = {"D": D, "utterances": n, "frames_per_utterance": T, "reps": reps, "g_kernel": "traj_g_mfma_kernel" if 2 * D <= 96 else "traj_g_kernel"}
    for m in modes:
        res[m] = {"call_ms": times[m], "call_median_ms": median(times[m]), "call_spread": (max(times[m]) - min(times[m])) / median(times[m]),
                  "frames_per_s": frames / (median(times[m]) * 1e-3)}
    if len(modes) == 2:
        res["full_over_diag"] = res["full"]["call_median_ms"] / res["diag"]["call_median_ms"]
        res["max_abs_difference_of_the_two_models"] = float((last["full"] - last["diag"]).abs().max())
    return res


def kernel_split(D, mode, n, T, reps):
    """per-kernel average durations (us) and calls of `reps` + 1 calls of one mode, traced in a child process"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--", sys.executable,
               os.path.abspath(__file__), "--dims", str(D), "--only", mode, "--utts", str(n), "--frames", str(T), "--reps", str(reps),
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
    ap.add_argument("--only", default=None, choices=MODES, help="one mode only (the traced child of --kernels)")
    ap.add_argument("--kernels", action="store_true", help="add the per-kernel split from a traced child process per (dimension, mode)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import _lib
    import bench
    assert torch.cuda.is_available(), "traj_diag_bench needs a HIP device (there is no CPU fallback)"
    dims = [int(d) for d in a.dims.split(",")]
    modes = (a.only,) if a.only else MODES
    out = {"tool": "traj_diag_bench", "M": M, "device": torch.cuda.get_device_name(0), "source_hash": bench.source_hash(),
           "args": {k: v for k, v in vars(a).items() if k != "out"},
           "results": [measure(vc, _lib, torch, D, a.utts, a.frames, a.reps, a.warmup, modes) for D in dims]}
    if a.kernels:
        for r in out["results"]:
            for m in modes:
                r[m]["kernels"] = kernel_split(r["D"], m, a.utts, a.frames, min(a.reps, 3))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
