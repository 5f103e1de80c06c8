"""One EM iteration (E-step statistics + M-step) on frames drawn from a cross-diagonal model, at Dj = 80, M = 64 on 1.25e6
frames and Dj = 160, M = 64 on 5e5 frames, through the three device-resident states on the SAME frames:

  block_diag_ms  BlockDiagEMState (vcmi_gmm_em_bdiag_*), the model itself;
  diag_ms        DiagEMState on its variances (the cross-covariances dropped): the cheaper model that cannot convert;
  full_ms        EMState on the expanded (Dj,Dj,M) model: the only route to these statistics without the block-diagonal state.

Each figure is the median over R repetitions of the wall clock of K iterations (after W warm-up iterations of that state),
the device drained at the end of every timed block; the repetitions of the three states alternate, and the spread
(max - min) / median of each is reported with it.  fp64_roof_fraction: the NOMINAL products of the block-diagonal E-step per
frame and mixture -- 7 D on the vector pipe for the log-density, 5 D on v_mfma_f64_16x16x4_f64 for the statistics, 2 flop
each -- over block_diag_ms and the FP64 peak (--peak-tflops, 78.6 by default: MI355X vector = matrix FP64).  Nominal: the
statistics kernel skips k-steps whose 64 responsibilities are all exactly 0, so on separated mixtures it issues fewer; and it
is an end-to-end figure of the iteration (four launches per 131 072 frames and the M-step's host wait), not a kernel's.
--only full runs on a tree that has no block-diagonal state (the parent of the change that added it).  Prints one JSON line.
Usage: python tools/em_bdiag_bench.py [--shapes 80:64:1250000,160:64:500000] [--warmup W] [--steps K] [--reps R] [--only a,b]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model_and_frames(Dj, M, N, seed=4004):
    """w (M,), mu (Dj,M), covars (Dj + D, M), X (N,Dj): variances log-uniform in [1e-3, 1], pair correlations in (-0.9, 0.9),
    means N(0,1) -- separated mixtures, as the frames of a trained model are"""
    rng = np.random.default_rng(seed)
    D = Dj // 2
    w = rng.dirichlet(4.0 * np.ones(M))
    mu = rng.standard_normal((Dj, M))
    var = np.exp(rng.uniform(np.log(1e-3), 0.0, (Dj, M)))
    rho = rng.uniform(-0.9, 0.9, (D, M))
    cov = np.vstack([var, rho * np.sqrt(var[:D] * var[D:])])
    comp = rng.choice(M, size=N, p=w)
    X = np.empty((N, Dj))
    for lo in range(0, N, 1 << 17):
        c = comp[lo:lo + (1 << 17)]
        z1, z2 = rng.standard_normal((len(c), D)), rng.standard_normal((len(c), D))
        r = rho.T[c]
        X[lo:lo + len(c), :D] = mu[:D].T[c] + np.sqrt(var[:D]).T[c] * z1
        X[lo:lo + len(c), D:] = mu[D:].T[c] + np.sqrt(var[D:]).T[c] * (r * z1 + np.sqrt(1.0 - r * r) * z2)
    return w, np.asfortranarray(mu), np.asfortranarray(cov), X


def expand(cov):
    D, M = cov.shape[0] // 3, cov.shape[1]
    out = np.zeros((2 * D, 2 * D, M), order="F")
    for m in range(M):
        out[:, :, m] = np.diag(cov[:2 * D, m]) + np.diag(cov[2 * D:, m], D) + np.diag(cov[2 * D:, m], -D)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="80:64:1250000,160:64:500000")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="block_diag,diag,full")
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    a = ap.parse_args()
    import torch

    import voiceconversion_jl_amd as vc
    assert torch.cuda.is_available(), "em_bdiag_bench needs a HIP device (there is no CPU fallback)"
    kinds = a.only.split(",")
    out = {"tool": "em_bdiag_bench", "warmup": a.warmup, "steps": a.steps, "reps": a.reps, "results": []}
    for Dj, M, N in (tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")):
        w, mu, cov, Xh = model_and_frames(Dj, M, N)
        X = torch.from_numpy(Xh).cuda().t()
        del Xh
        make = {"block_diag": lambda: (vc.BlockDiagEMState(w, mu, cov), vc.bdiag_stats_len(Dj, M)),
                "diag": lambda: (vc.DiagEMState(w, mu, np.asfortranarray(cov[:Dj])), vc.stats_len(Dj, M)),
                "full": lambda: (vc.EMState(w, mu, expand(cov)), vc.full_stats_len(Dj, M))}
        runs = {}
        for k in kinds:
            em, n = make[k]()
            runs[k] = (em, torch.empty(n, dtype=torch.float64, device="cuda"), [])
            for _ in range(a.warmup):
                em.mstep(em.estep(X, out=runs[k][1]))
        torch.cuda.synchronize()
        for _ in range(a.reps):                       # the states alternate: drift of the machine reaches all of them
            for k in kinds:
                em, stats, ms = runs[k]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    em.estep(X, out=stats)
                    em.mstep(stats)
                torch.cuda.synchronize()
                ms.append(1e3 * (time.perf_counter() - t0) / a.steps)
        r = {"Dj": Dj, "M": M, "frames": N}
        for k in kinds:
            ms = runs[k][2]
            r[k + "_ms"] = float(np.median(ms))
            r[k + "_spread"] = float((max(ms) - min(ms)) / np.median(ms))
        if "block_diag" in kinds:
            flop = 2.0 * (7 + 5) * (Dj // 2) * float(M) * N
            r["nominal_gflop"] = flop / 1e9
            r["fp64_roof_fraction"] = flop / (r["block_diag_ms"] * 1e-3) / (a.peak_tflops * 1e12)
            for k in ("diag", "full"):
                if k in kinds:
                    r[f"{k}_over_block_diag"] = r[k + "_ms"] / r["block_diag_ms"]
        out["results"].append(r)
        del X, runs
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
