"""DiagTrajectoryGVGMMMap (the GV ascent over diagonal conditional precisions, csrc/traj_gv_band.hip) over a
BlockDiagTrajectoryGMMMap, against the only way to GV with a cross-diagonal model before it: the detour
TrajectoryGVGMMMap(TrajectoryGMMMap(GMMMap(w, mu, expand_block_diag(covars)), T), mu_v, Sigma_vv).  Device-resident.

  shapes:  M = 64, 100 epochs, alpha = 1e-5: 256 x 2000 frames at D = 40 and D = 59 (tools/traj_bdiag_bench.py's models and
           frames), and 5120 x 100 frames at D = 40 -- vc's default chunks; --shapes D:utts:frames,...
  timing:  HIP events around vcmi_trajgv_convert_batch_dev (the GV call) and vcmi_traj_convert_batch_dev on the converter under it
           (the plain call); the two paths ALTERNATE in one process: --rounds rounds of --calls consecutive calls per path and
           kind; per path and kind every time, the median and the spread (max - min) / median.  The GV part of a call is the
           GV call's median minus the plain call's; its spread is the two spreads (in ms) added.
  kernels: with --kernels every (shape, path) runs once more in a child process under `rocprofv3 --kernel-trace --stats`
           (tracing only, no counters), a run of its own; the GV kernel's average duration is added, and for traj_gvd_kernel the
           bytes it moves per epoch in the streamed form (four (T,D) arrays read, one written) against --peak-tbs
  form:    how many of the kernel's five arrays stay in LDS (csrc/traj_band_plan.hpp, restated here): 0 = streamed
  --root:  the tree whose package is imported (a checkout of another commit, with --only detour, measures the baseline there)

Usage: python tools/gv_diag_bench.py [--shapes 40:256:2000,59:256:2000,40:5120:100] [--rounds 5] [--calls 5] [--kernels] [--out FILE]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

M = 64
EPOCHS, ALPHA = 100, 1.0e-5
PATHS = ("diag", "detour")


def gvd_resident(D, Tmax):
    """csrc/traj_band_plan.hpp: band_resident over five arrays"""
    fit = (160 * 1024 - 256 - (2 * 512 + 3 * D) * 8) // (Tmax * D * 8)
    return 5 if fit >= 5 else (int(fit) if fit >= 2 else 0)


def median(v):
    return float(np.median(np.asarray(v)))


def build(vc, path, w, mu, cov, T):
    if path == "diag":
        return vc.BlockDiagTrajectoryGMMMap(vc.BlockDiagGMMMap(w, mu, cov), T)
    return vc.TrajectoryGMMMap(vc.GMMMap(w, mu, vc.expand_block_diag(cov)), T)


def measure(vc, lib, torch, tb, D, n, T, rounds, calls, warmup, paths):
    w, mu, cov = tb.model(D)
    rng = np.random.default_rng(1005)
    base = [tb.frames(vc, rng, w, mu, cov, T, D) for _ in range(min(n, 8))]
    Xd = torch.from_numpy(np.concatenate([base[i % len(base)] for i in range(n)])).cuda()
    Yd = torch.empty((n * T, D), dtype=torch.float64, device="cuda")
    xoff = np.arange(n, dtype=np.int64) * T * 2 * D
    yoff = np.arange(n, dtype=np.int64) * T * D
    Ts = np.full(n, T, dtype=np.int64)
    stream = torch.cuda.current_stream().cuda_stream
    traj = {p: build(vc, p, w, mu, cov, T) for p in paths}

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.check(f())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def plain(p):
        return timed(lambda: lib.lib.vcmi_traj_convert_batch_dev(traj[p]._h, n, Xd.data_ptr(), lib.iptr(xoff), lib.iptr(Ts), Yd.data_ptr(),
                                                                 lib.iptr(yoff), stream))

    # GV statistics from the plain trajectory of the first utterance: mu_v = 1.3 var_1, a dense asymmetric covariance
    plain(paths[0])
    y0 = Yd[:T].cpu().numpy()
    muv = y0.var(axis=0, ddof=1) * 1.3
    A = np.random.default_rng(D).standard_normal((D, D))
    Sv = A @ A.T / D * np.mean(muv) ** 2 * 0.1 + np.diag(muv ** 2 * 0.05)
    U = np.triu(Sv, 1)
    Sv = np.asfortranarray(Sv + 0.2 * (U - U.T))
    gvc = {p: (vc.DiagTrajectoryGVGMMMap if p == "diag" else vc.TrajectoryGVGMMMap)(traj[p], muv, Sv) for p in paths}

    def gv(p):
        return timed(lambda: lib.lib.vcmi_trajgv_convert_batch_dev(gvc[p]._h, n, Xd.data_ptr(), lib.iptr(xoff), lib.iptr(Ts), EPOCHS, ALPHA,
                                                                   Yd.data_ptr(), lib.iptr(yoff), stream))

    kinds = {"plain": plain, "gv": gv}
    for _ in range(warmup):
        for p in paths:
            for f in kinds.values():
                f(p)
    times = {(p, k): [] for p in paths for k in kinds}
    last = {}
    for _ in range(rounds):
        for p in paths:
            for k, f in kinds.items():
                for _ in range(calls):
                    times[(p, k)].append(f(p))
            if p not in last:
                last[p] = Yd.clone()          # (of the GV call)
    assert all(bool(torch.isfinite(y).all()) for y in last.values())
    res = {"D": D, "utterances": n, "frames_per_utterance": T, "rounds": rounds, "calls": calls, "epochs": EPOCHS, "alpha": ALPHA,
           "resident_arrays": gvd_resident(D, T)}
    for p in paths:
        r = {}
        for k in kinds:
            t = times[(p, k)]
            md = median(t)
            r[k] = {"call_ms": t, "median_ms": md, "spread": (max(t) - min(t)) / md}
        r["gv_part_ms"] = r["gv"]["median_ms"] - r["plain"]["median_ms"]
        r["gv_part_spread_ms"] = r["gv"]["spread"] * r["gv"]["median_ms"] + r["plain"]["spread"] * r["plain"]["median_ms"]
        res[p] = r
    if len(paths) == 2:
        a, b = res["diag"], res["detour"]
        res["gv_part_gain_ms"] = b["gv_part_ms"] - a["gv_part_ms"]
        res["spreads_combined_ms"] = a["gv_part_spread_ms"] + b["gv_part_spread_ms"]
        res["done"] = res["gv_part_gain_ms"] > res["spreads_combined_ms"]
        res["call_ratio_detour_over_diag"] = b["gv"]["median_ms"] / a["gv"]["median_ms"]
        res["max_rel_difference_of_the_two_results"] = float((last["diag"] - last["detour"]).abs().max() / last["detour"].abs().max())
    return res


def kernel_split(root, D, path, n, T):
    """per-kernel average durations (us) and calls of one path's calls, traced in a child process"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--", sys.executable,
               os.path.abspath(__file__), "--root", root, "--shapes", f"{D}:{n}:{T}", "--only", path, "--rounds", "1", "--calls", "2",
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
    ap.add_argument("--shapes", default="40:256:2000,59:256:2000,40:5120:100")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--only", default=None, choices=PATHS, help="one path only (the traced child of --kernels; a tree without the other)")
    ap.add_argument("--kernels", action="store_true", help="add the per-kernel split from a traced child process per (shape, path)")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is measured")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import _lib
    import bench
    import traj_bdiag_bench as tb
    assert torch.cuda.is_available(), "gv_diag_bench needs a HIP device (there is no CPU fallback)"
    paths = (a.only,) if a.only else PATHS
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    out = {"tool": "gv_diag_bench", "M": M, "device": torch.cuda.get_device_name(0), "source_hash": bench.source_hash(),
           "package": os.path.dirname(os.path.abspath(vc.__file__)), "args": {k: v for k, v in vars(a).items() if k != "out"},
           "results": [measure(vc, _lib, torch, tb, D, n, T, a.rounds, a.calls, a.warmup, paths) for D, n, T in shapes]}
    if a.kernels:
        for r in out["results"]:
            for p in paths:
                r[p]["kernels"] = ks = kernel_split(os.path.abspath(a.root), r["D"], p, r["utterances"], r["frames_per_utterance"])
                gvk = [v for k, v in ks.items() if "traj_gv" in k and isinstance(v, dict)]
                if gvk:
                    r[p]["gv_kernel_us"] = gvk[0]["avg_us"]
                    if p == "diag" and r["resident_arrays"] == 0:
                        gb = 5.0 * 8 * r["D"] * r["utterances"] * r["frames_per_utterance"] / 1e9
                        r[p]["gb_per_epoch"] = gb
                        r[p]["hbm_roof_fraction"] = gb * 1e9 * EPOCHS / (gvk[0]["avg_us"] * 1e-6) / (a.peak_tbs * 1e12)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
