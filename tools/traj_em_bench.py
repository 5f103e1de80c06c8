"""EM re-estimation of the trajectory (TrajectoryGMMMap(g, T, em_iters=n), csrc/traj_em.hip) beside the arg-max conversion of
the same input, device-resident (vcmi_traj_convert_batch_dev), one GPU, one process.

Inputs: cfg5 (static D = 40, M = 64, --utts x 2000 frames) with an OVERLAPPING synthetic model (every frame a blend: the table's
worst case) and a PEAKED one (bench.py's: no frame mixed), and the reference's trained model (D = 20, M = 32) on the golden X
tiled to the same number of frames.  Per input: ms of the arg-max call and of the EM call (--iters iterations), --reps repeats
each, alternated; ms per EM iteration split by hip events inside the library (vcmi_debug_traj_em_times: E-step, gbar, flag scan
+ count read + blend, pad + solve); the E-step kernel's share of the 78.6 TF/s FP64 MFMA roof by its algorithmic 4 M (2D)^2
flop per frame; mixed-frame fraction and table bytes; and the run-to-run spread ((max - min) / median).
Usage: python tools/traj_em_bench.py [--utts N] [--iters K] [--reps R] [--only overlap|peaked|fixture] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import synthdata as sd  # noqa: E402

ROOF = 78.6e12


def julia_model(w, mu, sig):
    return w, np.asfortranarray(mu.T), np.asfortranarray(np.transpose(sig, (2, 1, 0)))


def frames(model, D, T, nbase, seed):
    import voiceconversion_jl_amd as vc
    w, mu, sig = model
    rng = np.random.default_rng(seed)
    base = []
    for _ in range(nbase):
        st = sd.sample_frames(int(rng.integers(1 << 30)), w, mu, sig, T, 0, D)
        st = np.cumsum(st, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
        base.append(np.ascontiguousarray(vc.push_delta(np.asfortranarray(st.T)).T))
    return base


def measure(label, model, base, D, M, T, n, iters, reps):
    import torch
    import voiceconversion_jl_amd as vc
    from voiceconversion_jl_amd import _lib
    g = vc.GMMMap(*julia_model(*model))
    tj = vc.TrajectoryGMMMap(g, T)
    X = np.concatenate([base[i % len(base)] for i in range(n)])
    Xd = torch.from_numpy(X).cuda()
    Yd = torch.empty((n * T, D), dtype=torch.float64, device="cuda")
    xoff = np.arange(n, dtype=np.int64) * T * 2 * D
    yoff = np.arange(n, dtype=np.int64) * T * D
    Ts = np.full(n, T, dtype=np.int64)
    hook = _lib.lib.vcmi_debug_traj_em_times
    hook.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    hook.restype = C.c_int

    def call(k):
        tj.em_iters = k
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(_lib.lib.vcmi_traj_convert_batch_dev(tj._h, n, Xd.data_ptr(), _lib.iptr(xoff), _lib.iptr(Ts), Yd.data_ptr(),
                                                        _lib.iptr(yoff), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    call(0)
    call(iters)
    y_arg = None
    t0s, tes = [], []
    for _ in range(reps):
        t0s.append(call(0))
        if y_arg is None:
            y_arg = Yd.clone()
        tes.append(call(iters))
    moved = float((Yd - y_arg).abs().max() / y_arg.abs().max())
    hist = tj.em_history().tolist()
    # the split, in a run of its own (the events add one wait per iteration)
    out7 = (C.c_double * 8)()
    _lib.check(hook(tj._h, 1, out7))
    splits = []
    for _ in range(reps):
        call(iters)
        _lib.check(hook(tj._h, 1, out7))
        splits.append([out7[k] / iters for k in range(4)] + [out7[4] / max(out7[6], 1.0), out7[5], out7[7] / iters])
    _lib.check(hook(tj._h, 0, out7))
    sp = np.array(splits)
    med = np.median(sp, axis=0)
    med0, mede = float(np.median(t0s)), float(np.median(tes))
    flop = 4.0 * M * (2 * D) ** 2 * n * T
    return {"input": label, "D": D, "M": M, "utterances": n, "frames_per_utterance": T, "iters": iters, "reps": reps,
            "argmax_ms": t0s, "em_ms": tes, "argmax_median_ms": med0, "em_median_ms": mede,
            "argmax_spread": (max(t0s) - min(t0s)) / med0, "em_spread": (max(tes) - min(tes)) / mede,
            "ms_per_iteration_total": (mede - med0) / iters,
            "ms_per_iteration": {"estep": med[0], "gbar": med[1], "scan_count_blend": med[2], "pad_solve": med[3]},
            "ms_per_iteration_spread": {k: float((sp[:, i].max() - sp[:, i].min()) / max(med[i], 1e-30))
                                        for i, k in enumerate(("estep", "gbar", "scan_count_blend", "pad_solve"))},
            "estep_flop": flop, "estep_fraction_of_fp64_mfma_roof": flop / (med[0] * 1e-3) / ROOF if med[0] > 0 else None,
            "mixed_fraction": med[4], "table_bytes_max": med[5], "slices": med[6], "objective": hist,
            "max_rel_move_from_argmax": moved}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["overlap", "peaked", "fixture"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "traj_em_bench needs a HIP device (there is no CPU fallback)"
    D, M, T, n = 40, 64, a.frames, a.utts
    out = {"tool": "traj_em_bench", "device": torch.cuda.get_device_name(0), "fp64_mfma_roof_flops": ROOF, "results": []}
    if a.only in (None, "peaked"):
        model = sd.synth_model(1005, 4 * D, M, lam_lo=1e-3)
        out["results"].append(measure("cfg5 peaked synthetic", model, frames(model, D, T, min(n, 8), 1005), D, M, T, n, a.iters, a.reps))
    if a.only in (None, "overlap"):
        w, mu, sig = sd.synth_model(900 + D, 4 * D, M, lam_lo=0.5)
        model = (w, 0.02 * mu, sig)
        out["results"].append(measure("cfg5 overlapping synthetic", model, frames(model, D, T, min(n, 8), 940), D, M, T, n, a.iters, a.reps))
    if a.only in (None, "fixture"):
        z = np.load(os.path.join(ROOT, "tests", "golden", "model_clb_to_slt_gmm32_order40_diff.npz"))
        X = np.load(os.path.join(ROOT, "tests", "golden", "trajectory_fixture_model.npz"))["X"]
        model = (z["weights"], z["means"], z["covars"])
        base = [np.ascontiguousarray(np.tile(X, ((T + len(X) - 1) // len(X), 1))[:T])]
        out["results"].append(measure("trained model, golden X tiled", model, base, X.shape[1] // 2, len(z["weights"]), T, n, a.iters, a.reps))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
