"""sp2mc / mc2sp at the issue's sizes: D = order + 1 = 41, fftlen 1024 and 1025 (K = 513), alpha = 0.41.

Prints one JSON line with, per fftlen:
  * mc2sp_dev_ms / sp2mc_dev_ms: vcmi_mc2sp_dev / vcmi_sp2mc_dev over --frames frames (device tensors), device-event time
    averaged over K calls after W warm-up calls;
  * *_host_utt_ms / *_host_ms: the host-pointer entries (numpy in, numpy out: PCIe both ways) for one --utt-frame utterance
    and for --frames frames, best of K (fewer for the large call) after one warm-up;
  * each as a fraction of the binding roof max(bytes / 6.3 TB/s, padded MFMA flop / 78.6 TF) of the work (one read of the
    input, one write of the output; the host entries against the same device roof);
  * cpu_*_ms: the folded-matrix numpy form (exp(G mc), H log(sp)) on the CPUs (at most 16 BLAS threads) over --cpu-frames
    frames, scaled to --frames.
Usage: python tools/mgc_bench.py [--frames N] [--warmup W] [--steps K] [--cpu-frames N] [--no-gpu]"""
import argparse
import json
import os
import sys
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = str(min(16, int(os.environ.get(v, "16"))))
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mgc_restatement as mr  # noqa: E402

HBM, FP64_MFMA = 6.3e12, 78.6e12
D, ALPHA = 41, 0.41


def up(n, m):
    return (n + m - 1) // m * m


def roof_ms(T, K, which):
    byts = 8.0 * T * (K + D)
    flop = 2.0 * T * (up(K, 16) * up(D, 4) if which == "mc2sp" else up(D, 16) * up(K, 4))
    return 1e3 * max(byts / HBM, flop / FP64_MFMA), ("bytes" if byts / HBM > flop / FP64_MFMA else "flop")


def dev_time(fn, warmup, steps):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def host_time(fn, reps):
    fn()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return 1e3 * best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--utt-frames", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cpu-frames", type=int, default=100_000)
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    T = a.frames
    mc = mr.smooth_mc(1, D, T, c0=-4.0)
    out = {"tool": "mgc_bench", "frames": T, "D": D, "alpha": ALPHA, "warmup": a.warmup, "steps": a.steps, "results": []}
    if not a.no_gpu:
        import torch
        import voiceconversion_jl_amd as vc
        assert torch.cuda.is_available(), "mgc_bench needs a HIP device (there is no CPU fallback)"
        dmc = torch.from_numpy(np.ascontiguousarray(mc.T)).cuda().t()
    for fftlen in (1024, 1025):
        K = fftlen // 2 + 1
        r = {"fftlen": fftlen, "K": K}
        for which in ("mc2sp", "sp2mc"):
            r[f"roof_{which}_ms"], r[f"roof_{which}_bound"] = roof_ms(T, K, which)
        if not a.no_gpu:
            dsp = vc.mc2sp(dmc, ALPHA, fftlen)
            dmc2 = vc.sp2mc(dsp, D - 1, ALPHA)
            r["mc2sp_dev_ms"] = dev_time(lambda: vc.mc2sp(dmc, ALPHA, fftlen), a.warmup, a.steps)
            r["sp2mc_dev_ms"] = dev_time(lambda: vc.sp2mc(dsp, D - 1, ALPHA), a.warmup, a.steps)
            r["roundtrip_max_abs_mc"] = float((dmc2 - dmc).abs().max()) if fftlen % 2 == 0 else None
            u = a.utt_frames
            mcu, spu = mc[:, :u].copy(order="F"), dsp[:, :u].cpu().numpy()
            r["mc2sp_host_utt_ms"] = host_time(lambda: vc.mc2sp(mcu, ALPHA, fftlen), a.steps)
            r["sp2mc_host_utt_ms"] = host_time(lambda: vc.sp2mc(spu, D - 1, ALPHA), a.steps)
            spT = dsp.cpu().numpy()
            del dsp, dmc2
            torch.cuda.empty_cache()
            reps = max(1, a.steps // 10)
            r["mc2sp_host_ms"] = host_time(lambda: vc.mc2sp(mc, ALPHA, fftlen), reps)
            r["sp2mc_host_ms"] = host_time(lambda: vc.sp2mc(spT, D - 1, ALPHA), reps)
            del spT
            for which in ("mc2sp", "sp2mc"):
                for kind in ("dev", "host"):
                    r[f"{which}_{kind}_frac_of_roof"] = r[f"roof_{which}_ms"] / r[f"{which}_{kind}_ms"]
        # CPU baseline: the folded matrices (from the restatement: G = log mc2sp(I), H = sp2mc(exp(I))), numpy + BLAS
        G = np.log(mr.mc2sp(np.eye(D), ALPHA, fftlen))
        H = mr.sp2mc(np.exp(np.eye(K)), D - 1, ALPHA)
        n = min(a.cpu_frames, T)
        mcc = np.ascontiguousarray(mc[:, :n])
        t0 = time.perf_counter()
        spc = np.exp(G @ mcc)
        t1 = time.perf_counter()
        H @ np.log(spc)
        t2 = time.perf_counter()
        r["cpu_mc2sp_ms"] = 1e3 * (t1 - t0) * T / n
        r["cpu_sp2mc_ms"] = 1e3 * (t2 - t1) * T / n
        r["cpu_frames_timed"] = n
        out["results"].append(r)
    out["cpu_threads"] = int(os.environ["OMP_NUM_THREADS"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
