"""The GV ascent of TrajectoryGVGMMMap at a static dimension above 48 (traj_gvw_kernel) beside the D = 40 kernel
(traj_gv2_kernel), device-resident.

  shape:  M = 64, 256 utterances x 2000 frames cut into chunks of L = 100 frames (bin/vc.jl:18), epochs = 100 -- what
          vc(tgv, fm) of order-59 mel-cepstra at 48 kHz runs at the CLI defaults -- through vcmi_trajgv_convert_batch_dev
  timing: HIP events around the entry, after warm-up calls; per dimension the calls with epochs = 100 and with epochs = 0
          (solve + the eq. (58) rescaling only) ALTERNATE, and the GV part is the difference of the two medians

Per dimension the JSON line holds every time, the medians, the spread of the repeats ((max - min) / median), frames/s of the
whole call, the GV part in ms and per frame-epoch, and the fraction of the FP64 MFMA roof (78.6 TFLOP/s) that the ISSUED
products of the ascent reach: per 16-frame tile NT row tiles x (k chunks x k-steps per chunk) v_mfma_f64_16x16x4 of 2048 flop,
with at least ceil(L / 16) tiles per chunk (the tiles are formed per mixture, so there are a few more).  Last, the cost per
frame-epoch of the wide dimension relative to D = 40, beside the (2D)^2 ratio.
Usage: python tools/gv_wide_bench.py [--dims 59,40] [--utts 256] [--frames 2000] [--chunk 100] [--epochs 100] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import synthdata as sd  # noqa: E402

M = 64
FP64_PEAK_TFLOPS = 78.6
ALPHA = 1.0e-5
KC, ROWS_PASS = 16, 12          # kGvwKC, kGvwRowsPass (csrc/traj_gv.hip)


def median(v):
    return float(np.median(np.asarray(v)))


def issued_mfma_per_tile(D):
    """v_mfma_f64_16x16x4 the ascent issues per 16-frame tile and epoch"""
    NT, KS = (2 * D + 15) // 16, (2 * D + 3) // 4
    if NT <= 6:
        return NT * KS                                  # traj_gv2_kernel: one wave per row tile, every k-step
    NC = (KS + KC - 1) // KC
    return NT * NC * ((KS + NC - 1) // NC)              # traj_gvw_kernel: even k chunks, the last one may repeat a k-step


def measure(vc, lib, torch, D, n, T, L, epochs, reps, warmup):
    w, mu, sig = sd.synth_model(1005 + D, 4 * D, M, lam_lo=1e-3)
    g = vc.GMMMap(w, np.asfortranarray(mu.T), np.asfortranarray(np.transpose(sig, (2, 1, 0))))
    tj = vc.TrajectoryGMMMap(g, L)
    rng = np.random.default_rng(1005)
    base = []
    for _ in range(min(n, 8)):
        st = sd.sample_frames(int(rng.integers(1 << 30)), w, mu, sig, T, 0, D)
        st = np.cumsum(st, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
        base.append(np.ascontiguousarray(vc.push_delta(np.asfortranarray(st.T)).T))       # (T,2D)
    Xd = torch.from_numpy(np.concatenate([base[i % len(base)] for i in range(n)])).cuda()
    Yd = torch.empty((n * T, D), dtype=torch.float64, device="cuda")
    starts = [(u, b) for u in range(n) for b in range(0, T, L)]
    xoff = np.array([(u * T + b) * 2 * D for u, b in starts], dtype=np.int64)
    yoff = np.array([(u * T + b) * D for u, b in starts], dtype=np.int64)
    Ts = np.array([min(L, T - b) for _, b in starts], dtype=np.int64)
    y0 = np.ascontiguousarray(vc.fvconvert(tj, np.asfortranarray(base[0][:200].T)).T)     # GV statistics from a short conversion
    muv = y0.var(axis=0, ddof=1) * 1.3
    Ar = np.random.default_rng(7).standard_normal((D, D))
    tgv = vc.TrajectoryGVGMMMap(tj, muv, Ar @ Ar.T / D * np.mean(muv) ** 2 * 0.1 + np.diag(muv ** 2 * 0.05))
    stream = torch.cuda.current_stream().cuda_stream

    def call(ep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.check(lib.lib.vcmi_trajgv_convert_batch_dev(tgv._h, len(Ts), Xd.data_ptr(), lib.iptr(xoff), lib.iptr(Ts), ep, ALPHA,
                                                        Yd.data_ptr(), lib.iptr(yoff), stream))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        call(epochs)
        call(0)
    full, init = [], []
    for _ in range(reps):
        full.append(call(epochs))
        init.append(call(0))
    assert bool(torch.isfinite(Yd).all())
    frames = n * T
    gv_ms = median(full) - median(init)
    tiles = len(Ts) * ((L + 15) // 16)
    flop = 2048.0 * issued_mfma_per_tile(D) * tiles * epochs
    return {"D": D, "row_tiles": (2 * D + 15) // 16, "k_steps": (2 * D + 3) // 4, "kernel": "traj_gv2_kernel" if 2 * D <= 96 else "traj_gvw_kernel",
            "utterances": n, "frames_per_utterance": T, "chunk": L, "chunks": len(Ts), "epochs": epochs, "reps": reps,
            "call_ms": full, "call_epochs0_ms": init, "call_median_ms": median(full), "call_epochs0_median_ms": median(init),
            "call_spread": (max(full) - min(full)) / median(full), "frames_per_s": frames / (median(full) * 1e-3),
            "gv_ms": gv_ms, "gv_ns_per_frame_epoch": gv_ms * 1e6 / (frames * epochs),
            "issued_mfma_per_tile_epoch": issued_mfma_per_tile(D), "issued_tflops": flop / (gv_ms * 1e-3) / 1e12,
            "fp64_mfma_roof_frac_issued": flop / (gv_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="59,40")
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import _lib
    import bench
    assert torch.cuda.is_available(), "gv_wide_bench needs a HIP device (there is no CPU fallback)"
    dims = [int(d) for d in a.dims.split(",")]
    out = {"tool": "gv_wide_bench", "M": M, "device": torch.cuda.get_device_name(0), "source_hash": bench.source_hash(),
           "args": {k: v for k, v in vars(a).items() if k != "out"}, "results": [measure(vc, _lib, torch, D, a.utts, a.frames, a.chunk, a.epochs, a.reps, a.warmup) for D in dims]}
    if len(dims) == 2:
        wide, ref = out["results"]
        out["cost_per_frame_epoch_ratio"] = wide["gv_ns_per_frame_epoch"] / ref["gv_ns_per_frame_epoch"]
        out["dim_squared_ratio"] = (wide["D"] / ref["D"]) ** 2
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
