"""CPU: tests/gmmmap_restatement.py before tests/test_gpu_gmmmap_shared.py judges the device by it.
  1. The longdouble restatement agrees with oracle/np_oracle.GMMMap and oracle/c_oracle.GMMMap inside the file's OWN bounds
     (log-densities, posteriors relatively, y element by element), on the reference's trained model and on tied_model, both
     swaps.  The float64 oracles are forms the bounds cover (centred whitening by substitution): an oracle that left a bound
     would show the bound wrong.
  2. The generators' claims, as conditions: on every shape the GPU module uses at least 90 % of tied_model's own frames have a
     second posterior >= 1e-3 (measured >= 99 %); in the harder setting at least 82 %, but for four shapes with few mixtures,
     (D, M) = (7, 3): 46 %, (75, 4): 68 %, (13, 3): 79 %, (50, 4): 81 %, held to 40 %; source_tied_ladder's source blocks are
     bitwise equal, its joint covariances positive definite, its weights reach from 0.73 down to 7e-305, and the oracles return
     the weight vector as every frame's posterior inside the bound."""
import numpy as np
import pytest
import scipy.linalg as sla

import gmmmap_restatement as rs

HARD_BELOW_82 = {(7, 3), (13, 3), (50, 4), (75, 4)}     # harder setting: shapes whose share of shared frames is 46-81 %
F64 = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731


def fractions(mdl, X, L=None, P=None, Y=None, prune=np.inf):
    """the largest |oracle - restatement| / bound for whichever of L, P, Y is given"""
    Yl, Pl, Ll = mdl.convert(X)
    out = {}
    with np.errstate(invalid="ignore"):               # (-inf against -inf and 0 / 0 of a mixture without weight: masked below)
        dL, dP = (None if L is None else np.abs(L - Ll)), (None if P is None else np.abs(P / Pl - 1))
    if L is not None:
        B = mdl.logdens_bound(X)
        live = np.isfinite(B)
        assert np.all(np.isneginf(L[~live])) and np.all(np.isneginf(F64(Ll)[~live]))
        out["L"] = float(np.max(dL[live] / B[live]))
    if P is not None:
        R, PB = mdl.posterior_bound(X, Pl)
        held = F64(Pl) >= 1e-300
        out["P"] = float(np.max(dP[held] / R[held]))
        out["Pabs"] = float(np.max(np.max(np.abs(P - Pl), axis=1) / PB))
    if Y is not None:
        out["Y"] = float(np.max(np.abs(Y - Yl) / mdl.convert_bound(X, prune)))
    return out


def posterior64(X, w, mu, sig, swap=False):
    """float64 posterior, vectorised (the generators' claims are about shares at 1e-3, not about rounding)"""
    D = mu.shape[1] // 2
    xs = slice(D, 2 * D) if swap else slice(0, D)
    L = np.empty((len(X), len(w)))
    for m in range(len(w)):
        C = np.linalg.cholesky(sig[m][xs, xs])
        Z = sla.solve_triangular(C, (X - mu[m, xs]).T, lower=True)
        L[:, m] = np.log(w[m]) - (D * np.log(2 * np.pi) + 2 * np.log(np.diag(C)).sum() + (Z * Z).sum(axis=0)) / 2
    return F64(rs.posterior(L))


@pytest.mark.parametrize("swap", [False, True])
def test_restatement_and_oracles_on_the_reference_model(fixture_model, swap):
    from oracle import c_oracle as co, np_oracle as npo
    w, mu, sig = fixture_model
    X = rs.frames(31, w, mu, sig, 60, swap)
    mdl = rs.Model(w, mu, sig, swap)
    gn, gc = npo.GMMMap(w, mu, sig, swap=swap), co.GMMMap(w, mu, sig, swap=swap)
    fn = fractions(mdl, X, np.stack([gn.log_weighted(x) for x in X]), gn.predict_proba(X), gn.fvconvert(X))
    fc = fractions(mdl, X, gc.logdens(X), gc.predict_proba(X), gc.fvconvert(X))
    print(f"reference model swap={swap}: numpy oracle {fn}, C oracle {fc}")
    assert max(fn.values()) <= 1.0 and max(fc.values()) <= 1.0
    Ll = mdl.logdens(X)
    assert np.array_equal(rs.predict(Ll), gc.predict(X)) and np.array_equal(rs.predict(Ll), gn.predict(X))


@pytest.mark.parametrize("setting", list(rs.SETTINGS))
@pytest.mark.parametrize("D,M,swap", [(7, 3, False), (40, 9, True), (25, 9, False), (48, 64, False), (57, 6, True), (80, 4, False),
                                      (100, 5, False), (160, 5, False)])
def test_oracles_stay_inside_the_bounds_on_tied_models(D, M, swap, setting):
    from oracle import c_oracle as co, np_oracle as npo
    w, mu, sig = rs.tied_model(100 + D + M, 2 * D, M, **rs.SETTINGS[setting])
    w = w.copy()
    if M >= 5:
        w[1] = 0.0                                    # a mixture without weight: -inf, posterior 0, no statement
        w /= w.sum()
    X = rs.frames(200 + D, w, mu, sig, 70, swap)
    mdl = rs.Model(w, mu, sig, swap)
    gc = co.GMMMap(w, mu, sig, swap=swap)
    Pc = gc.predict_proba(X)
    fc = fractions(mdl, X, gc.logdens(X), Pc, gc.fvconvert(X))
    gn = npo.GMMMap(w, mu, sig, swap=swap)
    fn = fractions(mdl, X[:16], None, gn.predict_proba(X[:16]), gn.fvconvert(X[:16]))
    print(f"tied {setting} D={D} M={M} swap={swap}: C oracle {fc}, numpy oracle {fn}")
    assert max(fc.values()) <= 1.0 and max(fn.values()) <= 1.0
    if M >= 5:
        assert np.all(Pc[:, 1] == 0.0) and np.all(F64(mdl.convert(X)[1])[:, 1] == 0.0)
    # where the restatement's margin exceeds the bound the oracle's index is the restatement's
    Ll = mdl.logdens(X)
    Ls = np.sort(F64(Ll), axis=1)
    clear = Ls[:, -1] - Ls[:, -2] > 2 * np.where(np.isfinite(mdl.logdens_bound(X)), mdl.logdens_bound(X), 0.0).max(axis=1)
    assert clear.mean() >= 0.99 and np.array_equal(gc.predict(X)[clear], rs.predict(Ll)[clear])


def test_tied_models_share_their_posteriors_on_every_gpu_shape():
    convert = rs.GENERIC_SHAPES + [(40, 9, 131)] + rs.TILE_SHAPES + rs.EIGHT_WAVE_SHAPES + rs.FALLBACK_SHAPES + rs.GROUPED_SHAPES
    posterior = [(D, M, 131) for D, M in rs.POSTERIOR_TIED_SHAPES]
    worst = {}
    for setting, kw in rs.SETTINGS.items():
        for D, M, T in convert + (posterior if setting == "default" else []):
            w, mu, sig = rs.tied_model(100 + D + M, 2 * D, M, **kw)
            s2, s3 = rs.shared_frames(posterior64(rs.frames(200 + D, w, mu, sig, T), w, mu, sig))
            worst[setting] = min(worst.get(setting, 1.0), s2)
            assert s2 >= (0.9 if setting == "default" else (0.4 if (D, M) in HARD_BELOW_82 else 0.82)), (setting, D, M, s2)
            if setting == "default" and M >= 9:
                assert s3 >= 0.9, (D, M, s3)
    print(f"smallest share of frames with a second posterior >= 1e-3: {worst}")


@pytest.mark.parametrize("D", [7, 40, 56, 100])
def test_source_tied_ladder(D):
    from oracle import c_oracle as co, np_oracle as npo
    for name, gaps in list(rs.LADDER_ORDERS.items()) + [("issue", rs.LADDER_GAPS), ("tied", rs.LADDER_TIED), ("long", rs.ladder_gaps(17))]:
        w, mu, sig = rs.source_tied_ladder(500 + D, D, gaps)
        M = len(gaps)
        assert w.max() > 0.2 and 2.3e-308 < w.min() < 1e-300          # the smallest weight is still a normal number
        for m in range(1, M):
            assert mu[m, :D].tobytes() == mu[0, :D].tobytes() and sig[m, :D, :D].tobytes() == sig[0, :D, :D].tobytes()
            assert not np.array_equal(mu[m, D:], mu[0, D:])
        for m in range(M):
            assert np.array_equal(sig[m], sig[m].T) and np.linalg.eigvalsh(sig[m]).min() > 0
        X = rs.frames(600 + D, w, mu, sig, 24)
        mdl = rs.Model(w, mu, sig)
        Pw = rs.ladder_posterior(w)
        R, _ = mdl.posterior_bound(X, np.broadcast_to(Pw, (len(X), M)))
        # the restatement's own softmax returns the weights to longdouble rounding; the oracles inside the bound
        assert np.max(np.abs(mdl.convert(X)[1] / Pw - 1)) < 1e-15
        for g in (co.GMMMap(w, mu, sig), npo.GMMMap(w, mu, sig)):
            Xo = X if isinstance(g, co.GMMMap) else X[:6]
            f = np.abs(g.predict_proba(Xo) / Pw - 1) / R[:len(Xo)]
            assert np.all(f <= 1.0), (name, float(f.max()))
            fy = np.abs(g.fvconvert(Xo) - rs.ladder_convert(Xo, w, mu, sig)) / mdl.convert_bound(Xo, np.inf)
            assert np.all(fy <= 1.0), (name, float(fy.max()))
        if name == "issue":
            rel = float(np.max(np.abs(npo.GMMMap(w, mu, sig).predict_proba(X[:6]) / Pw - 1)))
            print(f"D={D}: numpy oracle P / w - 1 <= {rel:.2e}; smallest relative bound {float(R.min()):.2e}, largest {float(R.max()):.2e}")
        if name == "tied":
            assert np.all(co.GMMMap(w, mu, sig).predict(X) == 2) and np.all(rs.predict(mdl.logdens(X)) == 2)
