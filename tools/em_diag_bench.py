"""One diagonal-covariance EM iteration per 1.25e6 frames at Dj = 80, M = 16, 32 and 128 (the estep workload's model and
frames: bench.py, bench_estep): E-step statistics + M-step, wall clock per iteration averaged over K iterations after W
warm-up iterations, the device drained at the end of the timed block.

  (a) device_ms: the device-resident loop -- DiagEMState.estep, DiagEMState.mstep (vcmi_gmm_em_diag_*); the parameters never
      leave HBM, the one host wait per iteration is the M-step's read of the log-likelihood and the flag;
  (b) hand_ms: the loop a user writes without it -- estep_diag_dev, .cpu(), estep.py:mstep_diag in numpy, the next
      estep_diag_dev with the new host parameters.
Both start from the same model, run the same number of iterations on the same frames and end on the same parameters to
rounding (max_rel_diff_means).  Prints one JSON line.
Usage: python tools/em_diag_bench.py [--frames N] [--warmup W] [--steps K] [--mixtures 16,32,128]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_250_000)
    ap.add_argument("--dj", type=int, default=80)
    ap.add_argument("--mixtures", default="16,32,128")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import torch

    import synthdata as npo
    import voiceconversion_jl_amd as vc
    assert torch.cuda.is_available(), "em_diag_bench needs a HIP device (there is no CPU fallback)"
    Dj, N = a.dj, a.frames
    out = {"tool": "em_diag_bench", "frames": N, "Dj": Dj, "warmup": a.warmup, "steps": a.steps, "results": []}
    for M in (int(m) for m in a.mixtures.split(",")):
        w, mu, _ = npo.synth_model(1003, Dj, M)
        var = np.exp(np.random.default_rng(1003).uniform(np.log(1e-3), 0.0, (M, Dj)))
        rg = np.random.default_rng(2003)
        comp = rg.choice(M, size=N, p=w)
        X = torch.from_numpy(mu[comp] + rg.standard_normal((N, Dj)) * np.sqrt(var[comp])).cuda().t()
        start = (w, np.asfortranarray(mu.T), np.asfortranarray(var.T))
        stats = torch.empty(vc.stats_len(Dj, M), dtype=torch.float64, device="cuda")

        def timed(iteration):
            for _ in range(a.warmup):
                iteration()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                iteration()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / a.steps

        em = vc.DiagEMState(*start)

        def device_iteration():
            em.estep(X, out=stats)
            em.mstep(stats)

        p = list(start)

        def hand_iteration():
            st = vc.estep_diag_dev(X, *p, out=stats).cpu().numpy()
            S0, S1, S2, _ = vc.unpack_stats(st, Dj, M)
            p[:] = vc.mstep_diag(S0, S1, S2)

        r = {"M": M, "device_ms": timed(device_iteration), "hand_ms": timed(hand_iteration)}
        r["speedup"] = r["hand_ms"] / r["device_ms"]
        r["max_rel_diff_means"] = float(np.max(np.abs(em.get()[1] - p[1])) / np.max(np.abs(p[1])))
        out["results"].append(r)
        del X
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
