"""vc of a TrajectoryGMMMap with the VarianceScaling post-filter, from STATIC features: the two host-pointer paths side by side.

  today:  host push_delta (vcmi_push_delta) + the (2D+1,T) matrix [power; static; delta] assembled on the host
          + vcmi_vc_traj_postf                                   -- (2D+1) + (D+1) rows per frame over PCIe
  static: vcmi_vc_traj_static on the (D+1,T) matrix [power; static]  -- 2 (D+1) rows per frame over PCIe

One GPU, one process, the two paths ALTERNATED (today, static, today, static, ...) after one warm-up call of each, every call
into a reused output array; D = 40, M = 64, L = 100 at T = 2000 (an utterance) and T = 10^6 (halved while the device runs out
of memory).  Per size the JSON line holds every wall-clock time, the medians, the ratio static / today, the spread of today's
repeats ((max - min) / median) and whether static <= today (1 + spread) holds, beside the PCIe bytes of each path computed
from the shapes.  Usage: python tools/vc_static_bench.py [--frames N] [--utt-frames N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import synthdata as sd  # noqa: E402

D, M, L = 40, 64, 100


def median(v):
    return float(np.median(np.asarray(v)))


def measure(lib, model, tj, T, reps):
    rng = np.random.default_rng(T)
    w, mu, sig = model
    st = np.cumsum(sd.sample_frames(32, w, mu, sig, T, 0, D), axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
    fm_static = np.asfortranarray(np.vstack([np.linspace(0, 1, T)[None], st.T]))          # (D+1,T)
    del st
    s2 = rng.uniform(0.5, 2.0, D)
    X = np.empty((2 * D, T), order="F")
    fm = np.empty((2 * D + 1, T), order="F")
    out_today, out_static = np.empty((D + 1, T), order="F"), np.empty((D + 1, T), order="F")
    h, dp = tj._h, lib.dptr

    def today():
        t0 = time.perf_counter()
        static = np.asfortranarray(fm_static[1:])                                         # src[2:end,:], bin/vc.jl:77
        lib.check(lib.lib.vcmi_push_delta(dp(static), D, T, dp(X)))
        fm[0] = fm_static[0]
        fm[1:] = X
        t1 = time.perf_counter()
        lib.check(lib.lib.vcmi_vc_traj_postf(h, dp(fm), T, dp(s2), dp(out_today)))
        t2 = time.perf_counter()
        return 1e3 * (t2 - t0), 1e3 * (t1 - t0)

    def static():
        t0 = time.perf_counter()
        lib.check(lib.lib.vcmi_vc_traj_static(h, dp(fm_static), T, dp(s2), dp(out_static)))
        return 1e3 * (time.perf_counter() - t0)

    today()
    static()
    assert len(tj) == (T - 1) % L + 1 == L, "the chunk length must stay L between the calls"
    t_today, t_prep, t_static = [], [], []
    for _ in range(reps):
        a, p = today()
        t_today.append(a)
        t_prep.append(p)
        t_static.append(static())
    err = float(np.max(np.abs(out_static - out_today)) / np.max(np.abs(out_today)))
    spread = (max(t_today) - min(t_today)) / median(t_today)
    return {"frames": T, "reps": reps, "today_ms": t_today, "today_host_prep_ms": t_prep, "static_ms": t_static,
            "today_median_ms": median(t_today), "static_median_ms": median(t_static),
            "ratio_static_over_today": median(t_static) / median(t_today), "today_spread": spread,
            "static_not_slower_within_spread": bool(median(t_static) <= median(t_today) * (1.0 + spread)),
            "pcie_bytes_today": 8 * T * ((2 * D + 1) + (D + 1)), "pcie_bytes_static": 8 * T * 2 * (D + 1),
            "pcie_byte_ratio": 2 * (D + 1) / ((2 * D + 1) + (D + 1)), "max_rel_diff_between_paths": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--utt-frames", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import _lib
    assert torch.cuda.is_available(), "vc_static_bench needs a HIP device (there is no CPU fallback)"
    model = w, mu, sig = sd.synth_model(311, 4 * D, M, lam_lo=1e-3)
    g = vc.GMMMap(w, np.asfortranarray(mu.T), np.asfortranarray(np.transpose(sig, (2, 1, 0))))
    tj = vc.TrajectoryGMMMap(g, L)
    out = {"tool": "vc_static_bench", "D": D, "M": M, "L": L, "device": torch.cuda.get_device_name(0), "results": []}
    out["results"].append(measure(_lib, model, tj, a.utt_frames, a.reps))
    T = a.frames
    while True:
        try:
            out["results"].append(measure(_lib, model, tj, T, a.reps))
            break
        except (vc.VCMIError, MemoryError) as e:             # as many frames as the device takes
            if "memory" not in str(e).lower() or T <= a.utt_frames:
                raise
            tj = vc.TrajectoryGMMMap(g, L)
            T //= 2
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
