"""BlockDiagTrajectoryGVGMMMap over BlockDiagTrajectoryGMMMap(g, T, windows=3) (the GV ascent over three windows,
csrc/traj_gv_band.hip: traj_gvp_kernel) beside the two-window DiagTrajectoryGVGMMMap (traj_gvd_kernel) on the same tree, in the
protocol of tools/gv_diag_bench.py.  Device-resident.

  shapes:  M = 64, D = 40, 100 epochs, alpha = 1e-5: 256 x 2000 frames and 5120 x 100 frames -- vc's default chunks
           (tools/traj_bdiag_windows_bench.py's models and frames per window count); --shapes D:utts:frames,...
  timing:  HIP events around vcmi_trajgv_convert_batch_dev (the GV call) and vcmi_traj_convert_batch_dev on the converter under it
           (the plain call); the window counts ALTERNATE in one process: --rounds rounds of --calls consecutive calls per window
           count and kind; per window count and kind every time, the median and the spread (max - min) / median.  The GV part of a
           call is the GV call's median minus the plain call's; its spread is the two spreads (in ms) added.  The ratio of the two
           GV parts is reported to be recorded, not as a gate: a five-point stencil over six arrays against a three-point stencil
           over five -- about 6/5 of the streamed bytes.
  kernels: with --kernels every (shape, windows) runs once more in a child process under `rocprofv3 --kernel-trace --stats`
           (tracing only, no counters), a run of its own; the GV kernel's average duration is added, and in the streamed form the
           bytes it moves per epoch (three windows: five (T,D) arrays read, one written, 6 T D 8; two windows: four and one)
           against --peak-tbs
  form:    how many of the kernel's arrays stay in LDS (csrc/traj_band_plan.hpp, restated here): 0 = streamed

Usage: python tools/gv_penta_bench.py [--shapes 40:256:2000,40:5120:100] [--rounds 5] [--calls 5] [--kernels] [--out FILE]"""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

M = 64
EPOCHS, ALPHA = 100, 1.0e-5
ARRAYS = {2: 5, 3: 6}        # (T,D) arrays of the ascent per window count


def resident(W, D, Tmax):
    """csrc/traj_band_plan.hpp: band_resident over five arrays (W = 2) or six (W = 3)"""
    fit = (160 * 1024 - 256 - (2 * 512 + 3 * D) * 8) // (Tmax * D * 8)
    return ARRAYS[W] if fit >= ARRAYS[W] else (int(fit) if fit >= 2 else 0)


def measure(vc, lib, torch, wb, D, n, T, rounds, calls, warmup, windows):
    stream = torch.cuda.current_stream().cuda_stream
    yoff = np.arange(n, dtype=np.int64) * T * D
    Ts = np.full(n, T, dtype=np.int64)
    st = {}
    for W in windows:
        w, mu, cov = wb.model(D, W)
        conv = vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(w, mu, cov), T, windows=W)
        rng = np.random.default_rng(1005)
        base = [wb.frames(vc, rng, w, mu, cov, T, D, W) for _ in range(min(n, 8))]
        Xd = torch.from_numpy(np.concatenate([base[i % len(base)] for i in range(n)])).cuda()
        Yd = torch.empty((n * T, D), dtype=torch.float64, device="cuda")
        st[W] = [conv, Xd, Yd, np.arange(n, dtype=np.int64) * T * W * D, None]

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.check(f())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def plain(W):
        conv, Xd, Yd, xoff, _ = st[W]
        return timed(lambda: lib.lib.vcmi_traj_convert_batch_dev(conv._h, n, Xd.data_ptr(), lib.iptr(xoff), lib.iptr(Ts), Yd.data_ptr(),
                                                                 lib.iptr(yoff), stream))

    # GV statistics from the plain trajectory of the first utterance: mu_v = 1.3 var_1, a dense asymmetric covariance
    for W in windows:
        plain(W)
        y0 = st[W][2][:T].cpu().numpy()
        muv = y0.var(axis=0, ddof=1) * 1.3
        A = np.random.default_rng(D).standard_normal((D, D))
        Sv = A @ A.T / D * np.mean(muv) ** 2 * 0.1 + np.diag(muv ** 2 * 0.05)
        U = np.triu(Sv, 1)
        st[W][4] = (vc.BlockDiagTrajectoryGVGMMMap if W == 3 else vc.DiagTrajectoryGVGMMMap)(st[W][0], muv, np.asfortranarray(Sv + 0.2 * (U - U.T)))

    def gv(W):
        _, Xd, Yd, xoff, tgv = st[W]
        return timed(lambda: lib.lib.vcmi_trajgv_convert_batch_dev(tgv._h, n, Xd.data_ptr(), lib.iptr(xoff), lib.iptr(Ts), EPOCHS, ALPHA,
                                                                   Yd.data_ptr(), lib.iptr(yoff), stream))

    kinds = {"plain": plain, "gv": gv}
    for _ in range(warmup):
        for W in windows:
            for f in kinds.values():
                f(W)
    times = {(W, k): [] for W in windows for k in kinds}
    for _ in range(rounds):
        for W in windows:
            for k, f in kinds.items():
                for _ in range(calls):
                    times[(W, k)].append(f(W))
    assert all(bool(torch.isfinite(st[W][2]).all()) for W in windows)
    res = {"D": D, "utterances": n, "frames_per_utterance": T, "rounds": rounds, "calls": calls, "epochs": EPOCHS, "alpha": ALPHA}
    for W in windows:
        r = {"resident_arrays": resident(W, D, T)}
        for k in kinds:
            t = times[(W, k)]
            md = float(np.median(t))
            r[k] = {"call_ms": t, "median_ms": md, "spread": (max(t) - min(t)) / md}
        r["gv_part_ms"] = r["gv"]["median_ms"] - r["plain"]["median_ms"]
        r["gv_part_spread_ms"] = r["gv"]["spread"] * r["gv"]["median_ms"] + r["plain"]["spread"] * r["plain"]["median_ms"]
        res[f"windows{W}"] = r
    if len(windows) == 2:
        res["gv_part_windows3_over_windows2"] = res["windows3"]["gv_part_ms"] / res["windows2"]["gv_part_ms"]
    return res


def kernel_split(D, W, n, T):
    """per-kernel average durations (us) and calls of one window count's calls, traced in a child process"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--", sys.executable,
               os.path.abspath(__file__), "--shapes", f"{D}:{n}:{T}", "--only", str(W), "--rounds", "1", "--calls", "2", "--warmup", "1"]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=d, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return {"error": (p.stderr or p.stdout)[-400:]}
        rows = list(csv.DictReader(open(files[0])))
    return {r["Name"].split("(")[0][-60:]: {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "percent": float(r["Percentage"])}
            for r in rows[:8]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="40:256:2000,40:5120:100")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
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
    import traj_bdiag_windows_bench as wb
    assert torch.cuda.is_available(), "gv_penta_bench needs a HIP device (there is no CPU fallback)"
    windows = (a.only,) if a.only else (2, 3)
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    out = {"tool": "gv_penta_bench", "M": M, "device": torch.cuda.get_device_name(0), "source_hash": bench.source_hash(),
           "args": {k: v for k, v in vars(a).items() if k != "out"},
           "results": [measure(vc, _lib, torch, wb, D, n, T, a.rounds, a.calls, a.warmup, windows) for D, n, T in shapes]}
    if a.kernels:
        for r in out["results"]:
            for W in windows:
                rw = r[f"windows{W}"]
                rw["kernels"] = ks = kernel_split(r["D"], W, r["utterances"], r["frames_per_utterance"])
                gvk = [v for k, v in ks.items() if ("traj_gvp" in k or "traj_gvd" in k) and isinstance(v, dict)]
                if gvk:
                    rw["gv_kernel_us"] = gvk[0]["avg_us"]
                    if rw["resident_arrays"] == 0:
                        gb = ARRAYS[W] * 8.0 * r["D"] * r["utterances"] * r["frames_per_utterance"] / 1e9
                        rw["gb_per_epoch"] = gb
                        rw["hbm_roof_fraction"] = gb * 1e9 * EPOCHS / (gvk[0]["avg_us"] * 1e-6) / (a.peak_tbs * 1e12)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
