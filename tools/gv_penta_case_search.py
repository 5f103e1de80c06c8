#!/usr/bin/env python3
"""Grid search, on the CPU alone, for the (alpha, GV covariance scale) of every case of tests/gv_penta_restatement.py (the GV
ascent over three windows): tools/gv_diag_case_search.py's search -- alpha in {1, 3} 10^k, scale in 10^k, against the conditions of
tests/gv_restatement.py: both gradient summands >= 0.2 of every checked step for n >= 1, the step >= 1e-5 of max |y|, y finite and
within 10 max |y_0| over the run.  Among the settings that pass, the one whose smaller summand share is largest.  Prints the
SETTINGS and BATCH_SETTING tables of that file.

    python tools/gv_penta_case_search.py [--batch-only]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gv_penta_restatement as gp  # noqa: E402

ALPHAS = [m * 10.0 ** k for k in range(-4, 5) for m in (1.0, 3.0)]
SCALES = [10.0 ** k for k in range(-5, 3)]


def score(case):
    """the smallest summand share over the checked steps n >= 1, or None where a condition fails"""
    inp = gp.inputs(case)
    p, y0 = inp["pieces"], inp["y0"]
    top = float(np.max(np.abs(y0)))
    y = np.asarray(y0, dtype=gp.LD)
    worst = 1.0
    with np.errstate(all="ignore"):
        for n in range(max(case.ns) + 1):
            lik, gv = gp.gradient(p, y)
            if n in case.ns:
                dy = float(np.max(np.abs(lik + gv)))
                if not np.isfinite(dy) or dy == 0.0:
                    return None
                sg, sl = float(np.max(np.abs(gv))) / dy, float(np.max(np.abs(lik))) / dy
                if sl < 0.2 or case.alpha * dy < 1e-5 * float(np.max(np.abs(y))) or (n >= 1 and sg < 0.2):
                    return None
                if n >= 1:
                    worst = min(worst, sg, sl)
            y = y + gp.LD(case.alpha) * (lik + gv)
            if not np.all(np.isfinite(y.astype(np.float64))) or float(np.max(np.abs(y))) > 10 * top:
                return None
    return worst


def best(make):
    found = None
    for scale in SCALES:
        for alpha in ALPHAS:
            s = [score(c) for c in make(alpha, scale)]
            if all(v is not None for v in s) and (found is None or min(s) > found[0]):
                found = (min(s), alpha, scale)
    return found


def main():
    print("SETTINGS = {")
    for D, M, seq, T, ns in ([] if "--batch-only" in sys.argv else gp.SHAPES):
        f = best(lambda a, sc: [gp.Case(D, M, seq, T, a, sc, ns)])
        assert f is not None, (D, M, T)
        print(f"    ({D}, {M}, {T}): ({f[1]:g}, {f[2]:g}),      # smaller share {f[0]:.2f}", flush=True)
    print("}")
    f = best(lambda a, sc: [gp.Case(12, 4, "runs", T, a, sc, gp.N_SHORT) for T in gp.BATCH_TS])
    assert f is not None
    print(f"BATCH_SETTING = ({f[1]:g}, {f[2]:g})      # smaller share {f[0]:.2f}")


if __name__ == "__main__":
    main()
