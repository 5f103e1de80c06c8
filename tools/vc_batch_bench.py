"""vc over a test set: vc_batch against the loop of vc calls (the only way to convert a set before vc_batch existed).

  trajectory converter, D = 40, M = 64, L = 100, STATIC input with the VarianceScaling post-filter, 256 utterances of 2000
  frames (the `traj` workload's shape) and of 300 frames (a short sentence): host matrices and device tensors;
  GMMMap (frame by frame), D = 40, M = 64, 256 x 300 frames with the post-filter: host matrices;
  n = 1: vc_batch of ONE 2000-frame utterance against the single call.

One GPU, one process.  Per pair: one warm-up call of each side, then the two sides ALTERNATED (loop, batch, loop, batch, ...);
a host clock around calls that end in a blocking download (host matrices) or in torch.cuda.synchronize() (device tensors).
Per pair the JSON line holds every wall-clock time, the medians, min and max of each side, the ratio loop / batch, and the
largest relative difference between the two sides' results.  Usage: python tools/vc_batch_bench.py [--utts N] [--reps R]
[--sizes 2000,300] [--out FILE]"""
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
POOL = 8          # distinct utterances generated per size; the set repeats them (as separate arrays)


def stats(v):
    v = np.asarray(v)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "all_ms": [float(x) for x in v]}


def alternate(loop, batch, reps, sync):
    """-> (loop times, batch times, last results of each) in ms; `sync` ends a timed window"""
    def timed(f):
        sync()
        t0 = time.perf_counter()
        r = f()
        sync()
        return 1e3 * (time.perf_counter() - t0), r

    timed(loop)
    timed(batch)
    tl, tb = [], []
    for _ in range(reps):
        a, rl = timed(loop)
        b, rb = timed(batch)
        tl.append(a)
        tb.append(b)
    return tl, tb, rl, rb


def report(name, n, T, tl, tb, rl, rb, to_numpy):
    diff = max(float(np.max(np.abs(to_numpy(a) - to_numpy(b))) / np.max(np.abs(to_numpy(a)))) for a, b in zip(rl[:4], rb[:4]))
    sl, sb = stats(tl), stats(tb)
    return {"case": name, "utterances": n, "frames_per_utterance": T, "loop": sl, "batch": sb,
            "ratio_loop_over_batch": sl["median_ms"] / sb["median_ms"], "frames_per_s_batch": n * T / (1e-3 * sb["median_ms"]),
            "max_rel_diff_between_sides": diff}


def static_set(model, n, T):
    w, mu, sig = model
    pool = []
    for k in range(min(POOL, n)):
        st = np.cumsum(sd.sample_frames(32 + k, w, mu, sig, T, 0, D), axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
        pool.append(np.vstack([np.linspace(0, 1, T)[None], st.T]))
    return [np.asfortranarray(pool[u % len(pool)].copy()) for u in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="2000,300")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import voiceconversion_jl_amd as vc
    assert torch.cuda.is_available(), "vc_batch_bench needs a HIP device (there is no CPU fallback)"
    n = a.utts
    model = w, mu, sig = sd.synth_model(311, 4 * D, M, lam_lo=1e-3)
    g2 = vc.GMMMap(w, np.asfortranarray(mu.T), np.asfortranarray(np.transpose(sig, (2, 1, 0))))
    tj = vc.TrajectoryGMMMap(g2, L)
    vs = vc.VarianceScaling(np.random.default_rng(2).uniform(0.5, 2.0, D))
    out = {"tool": "vc_batch_bench", "D": D, "M": M, "L": L, "device": torch.cuda.get_device_name(0), "results": []}

    def none():
        pass

    def ident(x):
        return x

    def dev_np(x):
        return x.cpu().numpy()

    for T in [int(s) for s in a.sizes.split(",")]:
        assert T % L == 0, "the loop must leave len(c) at L"
        fms = static_set(model, n, T)
        tl, tb, rl, rb = alternate(lambda: [vc.vc(tj, fm, postfilter=vs, delta=True) for fm in fms],
                                   lambda: vc.vc_batch(tj, fms, postfilter=vs, delta=True), a.reps, none)
        out["results"].append(report("trajectory, host matrices", n, T, tl, tb, rl, rb, ident))
        dfms = [torch.from_numpy(np.ascontiguousarray(fm.T)).cuda().t() for fm in fms]
        tl, tb, rl, rb = alternate(lambda: [vc.vc(tj, fm, postfilter=vs, delta=True) for fm in dfms],
                                   lambda: vc.vc_batch(tj, dfms, postfilter=vs, delta=True), a.reps, torch.cuda.synchronize)
        out["results"].append(report("trajectory, device tensors", n, T, tl, tb, rl, rb, dev_np))
        del dfms
        if T == 2000:        # n = 1: the batch entry must cost what the single call costs
            one = fms[:1]
            tl, tb, rl, rb = alternate(lambda: [vc.vc(tj, one[0], postfilter=vs, delta=True)],
                                       lambda: vc.vc_batch(tj, one, postfilter=vs, delta=True), 5 * a.reps, none)
            out["results"].append(report("trajectory, host matrices, n = 1", 1, T, tl, tb, rl, rb, ident))
        assert len(tj) == L
    # frame by frame: GMMMap over D = 40 rows
    wg, mug, sigg = sd.synth_model(312, 2 * D, M, lam_lo=1e-3)
    g = vc.GMMMap(wg, np.asfortranarray(mug.T), np.asfortranarray(np.transpose(sigg, (2, 1, 0))))
    T = 300
    fms = [np.asfortranarray(np.vstack([np.linspace(0, 1, T)[None], sd.sample_frames(50 + u % POOL, wg, mug, sigg, T, 0, D).T]))
           for u in range(n)]
    tl, tb, rl, rb = alternate(lambda: [vc.vc(g, fm, postfilter=vs) for fm in fms], lambda: vc.vc_batch(g, fms, postfilter=vs),
                               a.reps, none)
    out["results"].append(report("GMMMap, host matrices", n, T, tl, tb, rl, rb, ident))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
