"""BlockDiagTrajectoryGMMMap(g, T, windows=3) (static + delta + delta-delta: the pentadiagonal solver of csrc/traj_penta.hip)
beside the two-window converter on the same tree, device-resident, in the protocol of tools/traj_bdiag_bench.py.

  shapes:  M = 64, static D = 40, 256 utterances x 2000 frames and 5120 x 100 frames (--shapes); one cross-diagonal model per
           window count (Dj = 2 windows D, the recipe of tools/traj_bdiag_bench.py), frames a scaled cumulative sum of draws
           from it with their deltas (push_delta(order=windows - 1))
  timing:  HIP events around vcmi_traj_convert_batch_dev after warm-up calls; 5 rounds of 5 calls per window count, the calls of
           the two ALTERNATING in one process; per window count the median of the 25 calls, the medians of the rounds and the
           spread (max - min) / median of the 25
  kernels: with --kernels every (shape, windows) runs once more in a child process under `rocprofv3 --kernel-trace --stats`
           (tracing only: no counters): the split of a call into the fused arg-max + g_t pass (bdmap_kernel<3, .>) and the solve
           (traj_diag_solve_kernel / traj_penta_solve_kernel), and each one's share of the HBM roof (--peak-tbs, 8.0) from the
           bytes it must move per frame, W = windows:  pass: x read and g store, W D doubles each, and the 8-byte index;
           solve: g read (W D), the forward sweep's stores and the back substitution's loads of them (W D each: u, z for two
           windows; l1, l2, z/d for three), the y store (D) and the low word of the index.

Usage: python tools/traj_bdiag_windows_bench.py [--shapes 256x2000,5120x100] [--dim 40] [--kernels] [--out FILE]"""
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

M = 64
ROUNDS, CALLS = 5, 5


def model(D, W):
    """w (M,), mu (2 W D, M), covars (3 W D, M): tools/traj_bdiag_bench.py's recipe over W D features per side"""
    rng = np.random.default_rng(1005 + D + 1000 * (W - 2))
    Dh, Dj = W * D, 2 * W * D
    w = rng.dirichlet(4.0 * np.ones(M))
    mu = np.asfortranarray(0.7 / np.sqrt(Dj) * rng.standard_normal((Dj, M)))
    var = np.exp(rng.uniform(np.log(0.05), 0.0, (Dj, 1)) + 0.7 / np.sqrt(Dj) * rng.standard_normal((Dj, M)))
    rho = np.clip(rng.uniform(-0.9, 0.9, (Dh, 1)) + 0.3 / np.sqrt(Dh) * rng.standard_normal((Dh, M)), -0.9, 0.9)
    return w, mu, np.asfortranarray(np.vstack([var, rho * np.sqrt(var[:Dh] * var[Dh:])]))


def frames(vc, rng, w, mu, cov, T, D, W):
    """(T, W D): source-static draws of the model, cumulative sum scaled by 1/sqrt(t), with their deltas (and delta-deltas)"""
    comp = rng.choice(M, size=T, p=w)
    st = mu[:D].T[comp] + np.sqrt(cov[:D]).T[comp] * rng.standard_normal((T, D))
    st = np.cumsum(st, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
    return np.ascontiguousarray(vc.push_delta(np.asfortranarray(st.T), order=W - 1).T)


def measure(vc, lib, torch, D, n, T, windows, warmup):
    state = {}
    for W in windows:
        w, mu, cov = model(D, W)
        conv = vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(w, mu, cov), T, windows=W)
        rng = np.random.default_rng(1005)
        base = [frames(vc, rng, w, mu, cov, T, D, W) for _ in range(min(n, 8))]
        Xd = torch.from_numpy(np.concatenate([base[i % len(base)] for i in range(n)])).cuda()
        Yd = torch.empty((n * T, D), dtype=torch.float64, device="cuda")
        state[W] = (conv, Xd, Yd, np.arange(n, dtype=np.int64) * T * W * D)
    yoff = np.arange(n, dtype=np.int64) * T * D
    Ts = np.full(n, T, dtype=np.int64)
    stream = torch.cuda.current_stream().cuda_stream

    def call(W):
        conv, Xd, Yd, xoff = state[W]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.check(lib.lib.vcmi_traj_convert_batch_dev(conv._h, n, Xd.data_ptr(), lib.iptr(xoff), lib.iptr(Ts), Yd.data_ptr(),
                                                      lib.iptr(yoff), stream))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        for W in windows:
            call(W)
    times = {W: [[] for _ in range(ROUNDS)] for W in windows}
    for r in range(ROUNDS):
        for _ in range(CALLS):
            for W in windows:
                times[W][r].append(call(W))
    assert all(bool(torch.isfinite(state[W][2]).all()) for W in windows)
    res = {"D": D, "utterances": n, "frames_per_utterance": T}
    for W in windows:
        flat = [t for r in times[W] for t in r]
        md = float(np.median(flat))
        res[f"windows{W}"] = {"call_ms": times[W], "call_median_ms": md, "round_medians_ms": [float(np.median(r)) for r in times[W]],
                              "call_spread": (max(flat) - min(flat)) / md, "frames_per_s": n * T / (md * 1e-3)}
    if len(windows) == 2:
        res["windows3_over_windows2"] = res["windows3"]["call_median_ms"] / res["windows2"]["call_median_ms"]
    return res


def kernel_split(D, W, n, T, peak_tbs):
    """per-kernel average durations (us) of the calls of one window count, traced in a child process; the pass and the solve with
    their shares of the HBM roof"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--", sys.executable,
               os.path.abspath(__file__), "--dim", str(D), "--only", str(W), "--shapes", f"{n}x{T}", "--warmup", "1"]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=d, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return {"error": (p.stderr or p.stdout)[-400:]}
        rows = list(csv.DictReader(open(files[0])))
    ks = {r["Name"].split("(")[0][-60:]: {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "percent": float(r["Percentage"])}
          for r in rows[:8]}
    N = n * T
    out = {"kernels": ks}
    for name, v in ks.items():
        if "bdmap_kernel" in name:
            out["pass_us"] = v["avg_us"]
            out["pass_hbm_roof_fraction"] = (16.0 * W * D + 8.0) * N / (v["avg_us"] * 1e-6) / (peak_tbs * 1e12)
        if "_solve_kernel" in name:
            out["solve_us"] = v["avg_us"]
            out["solve_bytes_per_frame"] = 8.0 * (3 * W + 1) * D + 4.0
            out["solve_hbm_roof_fraction"] = out["solve_bytes_per_frame"] * N / (v["avg_us"] * 1e-6) / (peak_tbs * 1e12)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x2000,5120x100", help="utterances x frames, comma separated")
    ap.add_argument("--dim", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--only", type=int, default=None, choices=(2, 3), help="one window count only (the traced child of --kernels)")
    ap.add_argument("--kernels", action="store_true", help="add the per-kernel split from a traced child process per (shape, windows)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import _lib
    import bench
    assert torch.cuda.is_available(), "traj_bdiag_windows_bench needs a HIP device (there is no CPU fallback)"
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    windows = (a.only,) if a.only else (2, 3)
    out = {"tool": "traj_bdiag_windows_bench", "M": M, "device": torch.cuda.get_device_name(0), "source_hash": bench.source_hash(),
           "args": {k: v for k, v in vars(a).items() if k != "out"},
           "results": [measure(vc, _lib, torch, a.dim, n, T, windows, a.warmup) for n, T in shapes]}
    if a.kernels:
        for r in out["results"]:
            for W in windows:
                r[f"windows{W}"].update(kernel_split(r["D"], W, r["utterances"], r["frames_per_utterance"], a.peak_tbs))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
