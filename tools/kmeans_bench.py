"""Device k-means at the issue's sizes: Dj = 80, M = 64 and 128, 1.25e6 frames from synthdata.py.

Prints one JSON line with, per M:
  * assign_ms: one assignment pass (vcmi_kmeans_assign_dev: labels + distances + packed statistics), device-event time
    averaged over K calls after W warm-up calls;
  * kmeans_ms: a whole kmeans(n_init=1, max_iter=20, tol=0) (seeding included), host clock around a synchronised call,
    best of K after W warm-up runs;
  * each as a fraction of the binding roof max(bytes / 6.3 TB/s, flop / 78.6 TF) of the work (one read of X and the
    2 N Dj M cross-term flop per pass; 20 passes for the whole run, seeding not counted in the roof);
  * with --sklearn: scikit-learn KMeans(algorithm="lloyd", n_init=1, max_iter=20, tol=0) on the same frames on the CPUs
    (the CPU baseline; --no-gpu runs only that part).
Usage: python tools/kmeans_bench.py [--frames N] [--warmup W] [--steps K] [--sklearn] [--no-gpu]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import synthdata  # noqa: E402

HBM, FP64_MFMA = 6.3e12, 78.6e12


def frames(N, Dj, seed=5):
    w, mu, sig = synthdata.synth_model(seed, Dj, 32, lam_lo=1e-2)
    return synthdata.sample_frames(seed + 1, w, 2.0 * mu, sig, N, 0, Dj)


def roof_s(N, Dj, M, passes=1):
    return passes * max(8.0 * N * Dj / HBM, 2.0 * N * Dj * M / FP64_MFMA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_250_000)
    ap.add_argument("--dim", type=int, default=80)
    ap.add_argument("--clusters", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    N, Dj = a.frames, a.dim
    X = frames(N, Dj)
    out = {"tool": "kmeans_bench", "frames": N, "Dj": Dj, "warmup": a.warmup, "steps": a.steps, "results": []}
    if not a.no_gpu:
        import torch
        import voiceconversion_jl_amd as vc
        km = sys.modules["voiceconversion_jl_amd.kmeans"]
        assert torch.cuda.is_available(), "kmeans_bench needs a HIP device (there is no CPU fallback)"
        Xd = torch.from_numpy(X).cuda().t()
    for M in a.clusters:
        r = {"M": M, "roof_assign_ms": 1e3 * roof_s(N, Dj, M), "roof_bound": "flop" if 2.0 * M / FP64_MFMA > 8.0 / HBM else "bytes"}
        if not a.no_gpu:
            C0 = X[np.random.default_rng(M).choice(N, M, replace=False)].T
            st = km.KMeansState(Dj, M, C0)
            stats = torch.empty(km.kmeans_stats_len(Dj, M), dtype=torch.float64, device="cuda")
            for _ in range(a.warmup):
                st.assign(Xd, out=stats)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                st.assign(Xd, out=stats)
            e1.record()
            torch.cuda.synchronize()
            r["assign_ms"] = e0.elapsed_time(e1) / a.steps
            r["assign_frac_of_roof"] = r["roof_assign_ms"] / r["assign_ms"]
            times = []
            for i in range(a.warmup + max(1, a.steps // 10)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = vc.kmeans(Xd, M, n_init=1, max_iter=20, tol=0.0, seed=i)
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times.append(time.perf_counter() - t0)
            r["kmeans_ms"] = 1e3 * min(times)
            r["kmeans_n_iter"] = res["n_iter"]
            r["kmeans_frac_of_roof"] = 1e3 * roof_s(N, Dj, M, passes=res["n_iter"] + 1) / r["kmeans_ms"]
        if a.sklearn:
            from sklearn.cluster import KMeans
            t0 = time.perf_counter()
            KMeans(n_clusters=M, algorithm="lloyd", n_init=1, max_iter=20, tol=0.0, random_state=0).fit(X)
            r["sklearn_cpu_ms"] = 1e3 * (time.perf_counter() - t0)
            r["cpu_threads"] = os.cpu_count()
        out["results"].append(r)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
