"""CPU: the group radius of the screened fvconvert, host side (csrc/gmmmap_prepare.cpp: screen_radius_table, screen_radius_lmin;
csrc/gmmmap_handle.hpp: ScreenRadius), through the host-only hook `_lib.screen_radius_host`.

For a group g, another mixture m and lambda > 0:  |z_m(x)|^2 + lambda |z_g(x)|^2 >= c_gm(lambda) = d' inv(S_m + S_g / lambda) d  for
every x (d = mu_m - mu_g, S the source blocks), so l_m(x) < l_g(x) - prune whenever
|z_g(x)|^2 < R_gm = max_j (c_gm(lambda_j) - 2 (lc_m - lc_g + prune)) / (1 + lambda_j), and R_g = min_m R_gm less a rounding margin.

* the table and lmin = lc_g - R_g / 2 against a numpy restatement at 1e-9 relative (the margin is restated too: it is part of what
  the kernel compares against);
* the certificate itself by brute force on 10^5 points per model that are NOT only model draws: draws at one to three sigma, the
  minimisers of the quadratics scaled onto the boundary of the radius (the points the bound is tight at), points on the boundary in
  random directions, and points between the means -- no x with |z_g|^2 < R_g may have any l_m >= l_g - prune;
* prune in {0, 46, 200}; a zero-weight mixture; two identical mixtures (R <= 0: nothing is certified);
* tests/c/radius_check.cpp, a stand-alone program over the same host code, built with ASan + UBSan like tests/test_screen2_host.py.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, julia_model

LAMBDAS = 2.0 ** np.arange(-3, 4)
RTOL = 1e-9


@pytest.fixture(scope="module")
def lib():
    from voiceconversion_jl_amd import _lib
    return _lib


def _parts(w, mu, sig, D):
    S = np.stack([(s[:D, :D] + s[:D, :D].T) / 2.0 for s in sig])
    mux = mu[:, :D]
    with np.errstate(divide="ignore"):
        lc = np.log(w) - 0.5 * (D * np.log(2.0 * np.pi) + np.array([np.linalg.slogdet(s)[1] for s in S]))
    return S, mux, lc


def _np_table(S, mux, lc):
    M = len(lc)
    c = np.full((M, M, len(LAMBDAS)), np.nan)
    for g in range(M):
        for m in range(M):
            if m == g or not np.isfinite(lc[g]) or not np.isfinite(lc[m]):
                continue
            d = mux[m] - mux[g]
            for j, lam in enumerate(LAMBDAS):
                c[g, m, j] = d @ np.linalg.solve(S[m] + S[g] / lam, d)
    return c


def _np_lmin(c, S, mux, lc, prune):
    """screen_radius_lmin restated: the raw radius, then the rounding margin of csrc/gmmmap_prepare.cpp"""
    M, D = mux.shape
    u_norm = max(np.linalg.norm(np.linalg.inv(np.linalg.cholesky(s))) for s in S)
    lcmax = np.abs(lc[np.isfinite(lc)]).max()
    R0, R, lmin = np.full(M, -np.inf), np.full(M, -np.inf), np.full(M, np.inf)
    for g in range(M):
        if not np.isfinite(lc[g]):
            continue
        r0, cmax = 1e12, 0.0
        for m in range(M):
            if m == g or not np.isfinite(lc[m]):
                continue
            r0 = min(r0, np.max((c[g, m] - 2.0 * (lc[m] - lc[g] + prune)) / (1.0 + LAMBDAS)))
            cmax = max(cmax, c[g, m].max())
        R0[g] = r0
        if not r0 > 0.0:
            continue
        xmax = np.linalg.norm(mux[g]) + np.sqrt(r0) * np.sqrt(np.trace(S[g]))
        delta = 16.0 * (D + 3) * 2.0 ** -53 * u_norm * xmax
        E = 2.0 * (np.sqrt(cmax) + np.sqrt(r0)) * delta + 2.0 * delta ** 2 + 2.0 ** -40 * (cmax + r0 + 4.0 * lcmax + 2.0 * prune)
        R[g] = (r0 - 4.0 * E) * (1.0 - 2.0 ** -20)
        if R[g] > 0.0:
            lmin[g] = lc[g] - 0.5 * R[g]
    return R0, R, lmin


def _close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)), (a, b)
    assert np.array_equal(a[~np.isfinite(a)], b[~np.isfinite(b)], equal_nan=True)
    f = np.isfinite(a)
    assert np.all(np.abs(a[f] - b[f]) <= RTOL * np.abs(b[f])), float(np.max(np.abs(a[f] - b[f]) / np.abs(b[f])))


def _points(seed, S, mux, lc, R, n):
    """n points: a quarter each of model draws at 1..3 sigma, boundary points towards the minimisers of the pair quadratics, boundary
    points in random directions, points on the segments between two means (with a little noise)"""
    rng = np.random.default_rng(seed)
    M, D = mux.shape
    Ls = np.linalg.cholesky(S)
    live = np.flatnonzero(np.isfinite(lc))
    q = n // 4
    out = []
    g = rng.choice(live, q)
    out.append(mux[g] + rng.uniform(1.0, 3.0, (q, 1)) * np.einsum("nij,nj->ni", Ls[g], rng.standard_normal((q, D))))
    # argmin_x |z_m|^2 + lam |z_g|^2 = mu_g + inv(inv(S_m) + lam inv(S_g)) inv(S_m) d, moved along its ray from mu_g onto |z_g|^2 = t R_g
    Sinv = np.linalg.inv(S)
    rays = []
    for a in live:
        for b in live:
            if a != b and R[a] > 0.0:
                for lam in LAMBDAS:
                    v = np.linalg.solve(Sinv[b] + lam * Sinv[a], Sinv[b] @ (mux[b] - mux[a]))
                    rays.append((a, v / np.sqrt(v @ Sinv[a] @ v)))
    if rays:
        pick = rng.integers(0, len(rays), q)
        t = rng.uniform(0.5, 0.999999, q)
        out.append(np.stack([mux[rays[i][0]] + np.sqrt(t[k] * R[rays[i][0]]) * rays[i][1] for k, i in enumerate(pick)]))
    ok = np.flatnonzero(R > 0.0)
    if len(ok):
        g = rng.choice(ok, q)
        u = rng.standard_normal((q, D))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        out.append(mux[g] + np.sqrt(rng.uniform(0.0, 0.999999, (q, 1)) * R[g][:, None]) * np.einsum("nij,nj->ni", Ls[g], u))
    a, b = rng.choice(live, q), rng.choice(live, q)
    out.append(mux[a] + rng.uniform(0.0, 1.0, (q, 1)) * (mux[b] - mux[a]) + 1e-2 * rng.standard_normal((q, D)))
    return np.concatenate(out)


def _brute_force(S, mux, lc, R, prune, X):
    """(points inside some radius, worst l_m - (l_g - prune) over them): the second must be negative"""
    M, D = mux.shape
    U = np.linalg.inv(np.linalg.cholesky(S))
    Z2 = np.stack([(((X - mux[m]) @ U[m].T) ** 2).sum(1) for m in range(M)], axis=1)
    L = lc[None] - 0.5 * Z2
    inside, worst = 0, -np.inf
    for g in range(M):
        sel = Z2[:, g] < R[g]
        if not sel.any():
            continue
        inside += int(sel.sum())
        others = np.delete(L[sel], g, axis=1)
        worst = max(worst, float((others - (L[sel, g] - prune)[:, None]).max()))
    return inside, worst


@pytest.mark.parametrize("D", [16, 40])
def test_table_lmin_and_certificate(lib, D):
    import synthdata as sd
    M = 8
    w, mu, sig = sd.synth_model(7, 2 * D, M)
    S, mux, lc = _parts(w, mu, sig, D)
    c_np = _np_table(S, mux, lc)
    for prune in (0.0, 46.0, 200.0):
        c, R, lmin, frac = lib.screen_radius_host(*julia_model(w, mu, sig), prune=prune)
        _close(c, c_np)
        # c_mg(1 / lambda) = c_gm(lambda) / lambda: what lets one factorisation serve both orders of a pair
        assert np.allclose(np.transpose(c, (1, 0, 2))[:, :, ::-1][~np.isnan(c)], (c / LAMBDAS)[~np.isnan(c)], rtol=1e-9, atol=0.0)
        R0, R_np, lmin_np = _np_lmin(c_np, S, mux, lc, prune)
        _close(R, R_np)
        _close(lmin, lmin_np)
        assert np.all(R < R0)                                        # the margin takes something, always
        X = _points(100 + D, S, mux, lc, R, 100_000)
        inside, worst = _brute_force(S, mux, lc, R, prune, X)
        print(f"D = {D}, prune {prune}: R {R.min():.1f} .. {R.max():.1f}, profile frames inside {frac:.3f}, "
              f"{inside} of {len(X)} points inside a radius, worst l_m - (l_g - prune) = {worst:.3f}")
        if np.any(R > 0.0):
            assert inside > 20_000                                   # the test looks at something
        assert worst < 0.0
    # a larger prune certifies less
    Rs = [lib.screen_radius_host(*julia_model(w, mu, sig), prune=p)[1] for p in (0.0, 46.0, 200.0)]
    assert np.all(Rs[0] > Rs[1]) and np.all(Rs[1] > Rs[2])


def test_zero_weight_mixture(lib):
    import synthdata as sd
    D, M = 16, 8
    w, mu, sig = sd.synth_model(7, 2 * D, M)
    w = w.copy()
    w[3] = 0.0
    w /= w.sum()
    S, mux, lc = _parts(w, mu, sig, D)
    c, R, lmin, _ = lib.screen_radius_host(*julia_model(w, mu, sig), prune=46.0)
    assert lmin[3] == np.inf and not R[3] > 0.0                      # as a group: nothing is certified
    assert np.all(np.isnan(c[3])) and np.all(np.isnan(c[:, 3]))      # as a competitor: skipped
    R0, R_np, lmin_np = _np_lmin(_np_table(S, mux, lc), S, mux, lc, 46.0)
    _close(R, R_np)
    _close(lmin, lmin_np)
    inside, worst = _brute_force(S, mux, lc, R, 46.0, _points(5, S, mux, lc, R, 100_000))
    assert inside > 20_000 and worst < 0.0


def test_identical_mixtures_certify_nothing(lib):
    import synthdata as sd
    D, M = 16, 8
    w, mu, sig = sd.synth_model(7, 2 * D, M)
    mu, sig = mu.copy(), sig.copy()
    mu[1], sig[1] = mu[0], sig[0]
    _, R, lmin, _ = lib.screen_radius_host(*julia_model(w, mu, sig), prune=46.0)
    assert R[0] <= 0.0 and R[1] <= 0.0 and lmin[0] == np.inf and lmin[1] == np.inf
    assert np.all(R[2:] > 0.0)                                       # the others keep theirs


def test_host_code_under_asan_ubsan():
    csrc = os.path.join(ROOT, "voiceconversion.jl_amd", "csrc")
    out = os.path.join(ROOT, "oracle", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "radius_check_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "c", "radius_check.cpp")] + [os.path.join(csrc, f) for f in ("core.cpp", "hostpipe.cpp", "devgroup.cpp", "gmmmap_prepare.cpp")]
    link = ["-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-ldl", "-lpthread"]
    subprocess.run(cmd + ["-fsanitize=address,undefined", "-o", exe] + link, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and "radius_check: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
