"""GPU: BlockDiagGMMMap (csrc/gmmmap_bdiag.hip) -- frame-by-frame conversion with a cross-diagonal joint GMM.

References: the C oracle's GMMMap on the EXPANDED model (parity bar 1e-9, the TOL of tests/test_gpu_gmmmap.py) and the
longdouble restatement tests/gmmmap_bdiag_restatement.py with its derived bounds (tests/test_gmmmap_bdiag_host.py ties the two
together on the CPU).  Models: em_bdiag_restatement.bdiag_model(9000 + D + M, 2 D, M); frames: the source half (target half
under swap) of draw(9001 + T, ...)."""
import functools

import numpy as np
import pytest

from conftest import frame_relerr
import call_history as ch
import em_bdiag_restatement as eb
import gmmmap_bdiag_restatement as rs

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def dev(a):
    """(T,D) numpy -> (D,T) device tensor with unit stride along D"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().t()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(D, M, T, swap=False):
    """model, frames X (T,D) and the C oracle's results on the expanded model; made once, never written to"""
    from oracle import c_oracle as co
    w, mu, cov = eb.bdiag_model(9000 + D + M, 2 * D, M)
    Z = eb.draw(9001 + T, w, mu, cov, T)
    X = np.ascontiguousarray(Z[:, D:] if swap else Z[:, :D])
    g = co.GMMMap(w, np.ascontiguousarray(mu.T), np.ascontiguousarray(np.transpose(eb.expand(cov), (2, 1, 0))), swap=swap)
    out = dict(w=w, mu=mu, cov=cov, X=X, Y=g.fvconvert(X), P=g.predict_proba(X), idx=g.predict(X), L=g.logdens(X),
               A=np.stack([np.diag(a) for a in g.A], axis=1))
    for a in out.values():
        a.setflags(write=False)
    return out


# --------------------------------------------------------------------------------------------- parity with the C oracle
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("D,M,T", rs.PARITY_SHAPES + rs.SMALL_TILE_SHAPES)
def test_parity_with_the_oracle_on_the_expanded_model(vc, D, M, T, swap):
    c = case(D, M, T, swap)
    g = vc.BlockDiagGMMMap(c["w"], c["mu"], c["cov"], swap=swap)
    assert isinstance(g, vc.FrameByFrameConverter) and len(g) == 1
    assert (vc.dim(g), vc.ncomponents(g), vc.size(g)) == (D, M, (D, 1)) and len(g.px) == M
    XT = np.asfortranarray(c["X"].T)
    Y = vc.fvconvert(g, XT)
    P = vc.predict_proba(g.px, XT)
    idx = vc.predict(g.px, XT)
    ey, ep = frame_relerr(Y, c["Y"].T), float(np.max(np.abs(P - c["P"].T)))
    print(f"D={D} M={M} T={T} swap={swap}: frame-relative {ey:.2e}, posterior {ep:.2e}")
    assert Y.shape == (D, T) and P.shape == (M, T) and idx.shape == (T,) and idx.dtype == np.int64
    assert ey < TOL and ep < TOL
    if M > 1:                                              # no frame is left out: every margin of the ORACLE is clear
        Ls = np.sort(c["L"], axis=1)
        assert float(np.min(Ls[:, -1] - Ls[:, -2])) > 1e-6
    assert np.array_equal(idx, c["idx"])
    assert np.max(np.abs(g.slopes - c["A"])) <= 1e-12 * np.max(np.abs(c["A"]))
    # the reference's one-frame signature, out=, and the device entries
    y0 = vc.fvconvert(g, c["X"][0])
    assert y0.shape == (D,) and np.array_equal(y0, Y[:, 0])
    assert vc.predict(g.px, c["X"][0]) == idx[0] and np.array_equal(vc.predict_proba(g.px, c["X"][0]), P[:, 0])
    out = np.full((D, T), np.nan, order="F")
    assert vc.fvconvert(g, XT, out=out) is out and np.array_equal(out, Y)
    Xd = dev(c["X"])
    assert np.array_equal(host(vc.fvconvert(g, Xd)), Y)
    assert np.array_equal(host(vc.predict_proba(g.px, Xd)), P) and np.array_equal(host(vc.predict(g.px, Xd)), idx)


# ------------------------------------------------------------------------------------------- posteriors, relatively
@pytest.mark.parametrize("D,M", [(40, 7), (128, 256)])
def test_ladder_posteriors_are_the_weights(vc, D, M):
    """Mixtures with bit-identical source means and variances and weights proportional to exp(-(47, 0, 1, 20, 45, 300, 700))
    (repeated up to M): the posterior of every frame is the normalised weight vector itself, from 0.73 / repeats down to
    7e-305 / repeats, and is held RELATIVELY: |P / w - 1| <= B_tm + max_k B_tk + (M + 16) eps with the log-density bound of
    tests/gmmmap_bdiag_restatement.py.  (40, 7) runs the kernel's 64-frame tiles, (128, 256) its 32-frame ones."""
    T = 70
    gaps = np.array(([47.0, 0.0, 1.0, 20.0, 45.0, 300.0, 700.0] * (-(-M // 7)))[:M])
    _, mu1, cov1 = eb.bdiag_model(9100 + D, 2 * D, 1)
    rng = np.random.default_rng(9101 + D)
    w = np.exp(-gaps) / np.exp(-gaps).sum()
    mu, cov = np.asfortranarray(np.repeat(mu1, M, axis=1)), np.asfortranarray(np.repeat(cov1, M, axis=1))
    s = rng.uniform(1.0, 1.3, M)
    mu[D:] += rng.standard_normal((D, M))
    cov[D:2 * D] *= s * s                                  # target variances and cross terms scaled: the pair stays positive definite
    cov[2 * D:] *= s
    assert all(mu[:D, m].tobytes() == mu[:D, 0].tobytes() and cov[:D, m].tobytes() == cov[:D, 0].tobytes() for m in range(M))
    X = np.ascontiguousarray(eb.draw(9102 + D, w, mu, cov, T)[:, :D])
    B = rs.logdens_bound(X, w, mu, cov)
    R = B + B.max(axis=1, keepdims=True) + (M + 16) * rs.EPS
    wl = np.asarray(w, dtype=rs.LD)
    g = vc.BlockDiagGMMMap(w, mu, cov)
    P = vc.predict_proba(g.px, np.asfortranarray(X.T)).T
    assert np.all(P > 0) and P.min() < 1e-300
    f = np.abs(np.log(P.astype(rs.LD) / (wl / wl.sum()))) / R
    print(f"D={D} M={M}: largest relative posterior error / bound {float(f.max()):.3g}, bounds {R.min():.2e} ... {R.max():.2e}")
    assert np.all(f <= 1.0), float(f.max())
    assert np.array_equal(host(vc.predict_proba(g.px, dev(X))).T, P)


# ------------------------------------------------------------------------------------ where an expanded form cancels
def test_centred_log_density_where_the_expanded_form_cancels(vc):
    """Fractions of the bounds used, measured on an MI355X: see the printed line (posterior and y against the longdouble
    restatement; the uncorrected expanded form misses the posterior bound 2.4e5 times, tests/test_gmmmap_bdiag_host.py)."""
    w, mu, cov, Z = rs.cancellation_case()
    X = Z[:, :8]
    Yl, Pl, _ = rs.convert(X, w, mu, cov, False, rs.LD)
    PB, YB = rs.posterior_bound(X, w, mu, cov), rs.convert_bound(X, w, mu, cov)
    g = vc.BlockDiagGMMMap(w, mu, cov)
    XT = np.asfortranarray(X.T)
    P, Y = vc.predict_proba(g.px, XT).T, vc.fvconvert(g, XT).T
    fp = np.max(np.abs(P - Pl), axis=1) / PB
    fy = np.abs(Y - Yl) / YB
    print(f"fraction of the posterior bound used {float(fp.max()):.4f}, of the y bound {float(fy.max()):.4f}")
    assert np.all(fp <= 1.0), float(fp.max())
    assert np.all(fy <= 1.0), float(fy.max())


# ---------------------------------------------------------------------------------------------------------------- edges
def test_a_mixture_without_weight_has_posterior_zero(vc):
    c = case(25, 5, 130)
    w = c["w"].copy()
    w[2] = 0.0
    g = vc.BlockDiagGMMMap(w, c["mu"], c["cov"])
    keep = [0, 1, 3, 4]
    g4 = vc.BlockDiagGMMMap(w[keep], c["mu"][:, keep], c["cov"][:, keep])
    XT = np.asfortranarray(c["X"].T)
    P = vc.predict_proba(g.px, XT)
    assert np.all(P[2] == 0.0) and not np.any(vc.predict(g.px, XT) == 3)
    assert frame_relerr(vc.fvconvert(g, XT), vc.fvconvert(g4, XT)) < 1e-12
    assert np.max(np.abs(P[keep] - vc.predict_proba(g4.px, XT))) < 1e-12


def test_tiny_variances_and_nearly_singular_pairs(vc):
    """variances of 1e-7 and pair correlations of +-(1 - 1e-6): only vx and c / vx enter, nothing is close to singular here"""
    from oracle import c_oracle as co
    D, M, T = 6, 3, 200
    rng = np.random.default_rng(5)
    w = np.array([0.2, 0.3, 0.5])
    mu = np.asfortranarray(rng.standard_normal((2 * D, M)) * 1e-3)
    var = np.full((2 * D, M), 1e-7)
    rho = (1.0 - 1e-6) * np.where(np.arange(D) % 2 == 0, 1.0, -1.0)[:, None] * np.ones((1, M))
    cov = np.asfortranarray(np.vstack([var, rho * 1e-7]))
    X = np.ascontiguousarray(eb.draw(6, w, mu, cov, T)[:, :D])
    # (the oracle factorises the source block only, which is diagonal: it serves as the reference at this conditioning)
    ref = co.GMMMap(w, np.ascontiguousarray(mu.T), np.ascontiguousarray(np.transpose(eb.expand(cov), (2, 1, 0))))
    g = vc.BlockDiagGMMMap(w, mu, cov)
    XT = np.asfortranarray(X.T)
    assert frame_relerr(vc.fvconvert(g, XT), ref.fvconvert(X).T) < TOL
    assert np.max(np.abs(vc.predict_proba(g.px, XT) - ref.predict_proba(X).T)) < TOL


def test_frame_counts_around_the_tile(vc):
    import torch
    c = case(40, 64, 4099)
    g = vc.BlockDiagGMMMap(c["w"], c["mu"], c["cov"])
    Yr, Pr, Lr = rs.convert(c["X"][:65], c["w"], c["mu"], c["cov"])
    for T in (1, 63, 64, 65):
        XT = np.asfortranarray(c["X"][:T].T)
        assert frame_relerr(vc.fvconvert(g, XT), Yr[:T].T) < TOL
        assert np.max(np.abs(vc.predict_proba(g.px, XT) - Pr[:T].T)) < TOL
        assert np.array_equal(vc.predict(g.px, XT), rs.predict(Lr[:T]))
    e = np.empty((40, 0), order="F")
    assert vc.fvconvert(g, e).shape == (40, 0) and vc.predict_proba(g.px, e).shape == (64, 0) and vc.predict(g.px, e).shape == (0,)
    ed = torch.empty((0, 40), dtype=torch.float64, device="cuda").t()
    assert tuple(vc.fvconvert(g, ed).shape) == (40, 0) and tuple(vc.predict(g.px, ed).shape) == (0,)
    assert vc.vc(g, np.empty((41, 0), order="F")).shape == (41, 0)


# --------------------------------------------------------------------------------------------------- isolation and bits
def test_a_nan_frame_stays_alone(vc):
    c = case(25, 5, 130)
    g = vc.BlockDiagGMMMap(c["w"], c["mu"], c["cov"])
    XT = np.asfortranarray(c["X"].T)
    Y, P = vc.fvconvert(g, XT), vc.predict_proba(g.px, XT)
    Xn = XT.copy(order="F")
    Xn[7, 77] = np.nan
    Yn, Pn = vc.fvconvert(g, Xn), vc.predict_proba(g.px, Xn)
    others = np.arange(130) != 77
    assert np.all(np.isnan(Yn[:, 77])) and np.all(np.isnan(Pn[:, 77]))
    assert ch.same_bits(Yn[:, others], Y[:, others]) and ch.same_bits(Pn[:, others], P[:, others])
    assert vc.predict(g.px, Xn).shape == (130,)


def test_same_bits_whatever_ran_before(vc):
    import torch
    c = case(41, 17, 257)
    D, T = 41, 257
    g = vc.BlockDiagGMMMap(c["w"], c["mu"], c["cov"])
    XT = np.asfortranarray(c["X"].T)
    Xd = dev(c["X"])
    Y = host(vc.fvconvert(g, Xd))
    P = host(vc.predict_proba(g.px, Xd))
    assert ch.same_bits(host(vc.fvconvert(g, Xd)), Y)                       # two consecutive calls
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        Ys, Ps, Is = vc.fvconvert(g, Xd), vc.predict_proba(g.px, Xd), vc.predict(g.px, Xd)
    s.synchronize()
    assert ch.same_bits(host(Ys), Y) and ch.same_bits(host(Ps), P) and np.array_equal(host(Is), c["idx"])
    assert ch.same_bits(vc.fvconvert(g, XT), Y) and ch.same_bits(vc.predict_proba(g.px, XT), P)     # host entries
    # a fresh thread (new scratch) and a fresh handle
    assert ch.same_bits(ch.fresh(lambda: vc.fvconvert(vc.BlockDiagGMMMap(c["w"], c["mu"], c["cov"]), XT)), Y)
    a, b = 37, 203                                                          # off the 64-frame tile
    assert ch.same_bits(vc.fvconvert(g, np.asfortranarray(XT[:, a:b])), Y[:, a:b])
    assert ch.same_bits(host(vc.fvconvert(g, Xd[:, a:b])), Y[:, a:b])
    assert ch.same_bits(vc.predict_proba(g.px, np.asfortranarray(XT[:, a:b])), P[:, a:b])
    # the strided (D+1) input of vc against the dense matrix, on the host and on the device
    fm = np.asfortranarray(np.vstack([np.arange(T, dtype=np.float64)[None], XT]))
    out = vc.vc(g, fm)
    assert ch.same_bits(out[0], fm[0]) and ch.same_bits(out[1:], Y)
    fd = torch.from_numpy(np.ascontiguousarray(fm.T)).cuda()                # (T, D+1)
    od = torch.empty_like(fd)
    vc.fvconvert(g, fd[:, 1:].t(), out=od[:, 1:].t())
    assert ch.same_bits(host(od)[:, 1:].T, Y)


# ------------------------------------------------------------------------------------------------------- vc / vc_batch
def test_vc_and_vc_batch(vc):
    c = case(25, 5, 130)
    D = 25
    g = vc.BlockDiagGMMMap(c["w"], c["mu"], c["cov"])
    w, mu, cov = c["w"], c["mu"], c["cov"]
    lens = [0, 1, 2, 300, 2049]
    fms = []
    for u, T in enumerate(lens):
        X = eb.draw(700 + u, w, mu, cov, T)[:, :D] if T else np.empty((0, D))
        fms.append(np.asfortranarray(np.vstack([100.0 + np.arange(T, dtype=np.float64)[None], X.T])))
    vs = vc.VarianceScaling(np.exp(np.random.default_rng(3).uniform(-1.0, 1.0, D)))
    for fm in fms[2:]:
        plain, filt = vc.vc(g, fm), vc.vc(g, fm, postfilter=vs)
        assert ch.same_bits(plain[0], fm[0]) and ch.same_bits(filt[0], fm[0])
        assert ch.same_bits(plain[1:], vc.fvconvert(g, np.asfortranarray(fm[1:])))
        assert frame_relerr(filt[1:], vc.fvpostf(vs, plain[1:])) < 1e-12
    outs = vc.vc_batch(g, fms)
    for fm, o in zip(fms, outs):
        assert o.shape == fm.shape and ch.same_bits(o, vc.vc(g, fm))
    keep = [0, 2, 3, 4]                                    # (with a filter a one-frame utterance is refused)
    outs = vc.vc_batch(g, [fms[k] for k in keep], postfilter=vs)
    for k, o in zip(keep, outs):
        assert ch.same_bits(o, vc.vc(g, fms[k], postfilter=vs) if lens[k] else fms[k])
    with pytest.raises(vc.DimensionMismatch):
        vc.vc(g, fms[1], postfilter=vs)
    with pytest.raises(vc.DimensionMismatch):
        vc.vc_batch(g, fms, postfilter=vs)
    with pytest.raises(ValueError):
        vc.vc(g, fms[3], delta=True)
    assert ch.same_bits(vc.vc_batch(g, [fms[3]])[0], vc.vc(g, fms[3]))      # the handle is usable afterwards


# -------------------------------------------------------------------------------------------------------------- errors
def test_errors(vc):
    w, mu, cov = eb.bdiag_model(1, 10, 3)
    D = 5
    for swap in (False, True):
        for (d, m, row, val) in [(2, 1, 0, 0.0), (4, 0, 1, -1.0), (3, 2, 2, np.nan), (1, 2, 2, None)]:
            bad = cov.copy(order="F")
            bad[row * D + d, m] = 1.0001 * np.sqrt(bad[d, m] * bad[D + d, m]) if val is None else val
            with pytest.raises(vc.PosDefException, match=rf"pair \({d + 1},{m + 1}\)"):
                vc.BlockDiagGMMMap(w, mu, bad, swap=swap)
    with pytest.raises(vc.DimensionMismatch):
        vc.BlockDiagGMMMap(np.ones(2) / 2, np.zeros((258, 2)), np.ones((387, 2)))
    with pytest.raises(vc.DimensionMismatch):
        vc.BlockDiagGMMMap(np.ones(257) / 257, np.zeros((4, 257)), np.ones((6, 257)))
    g = vc.BlockDiagGMMMap(w, mu, cov)
    for X in (np.zeros(D + 1), np.zeros((D + 1, 4)), dev(np.zeros((4, D - 1)))):
        with pytest.raises(vc.DimensionMismatch):
            vc.fvconvert(g, X)
    with pytest.raises(vc.DimensionMismatch):
        vc.predict_proba(g.px, np.zeros((D + 1, 4)))
    with pytest.raises(vc.DimensionMismatch):
        vc.predict(g.px, np.zeros((D - 1, 4)))
    with pytest.raises(vc.DimensionMismatch):
        vc.vc(g, np.zeros((D, 4)))
    with pytest.raises(TypeError, match="expand_block_diag"):
        vc.TrajectoryGMMMap(g, 10)
    assert vc.fvconvert(g, np.zeros((D, 2))).shape == (D, 2)


# ------------------------------------------------------------------------------------------------ the point of the feature
def test_a_fitted_block_diag_model_converts_as_it_is(vc):
    """train_gmm(covariance_type="block_diag") -> BlockDiagGMMMap straight from the result, against GMMMap on the expanded
    covariances (Dj = 16, M = 3, 4000 frames, the fit of tests/test_gpu_em_bdiag.py section 10)."""
    Dj, M, N = 16, 3, 4000
    D = Dj // 2
    w0, mu0, cov0 = eb.bdiag_model(101, Dj, M, sep=6.0)
    Z = eb.draw(102, w0, mu0, cov0, N)
    r = vc.train_gmm(dev(Z), n_components=M, n_init=1, init="kmeans", n_iter=30, covariance_type="block_diag")
    g = vc.BlockDiagGMMMap(r["weights"], r["means"], r["covars"])
    gd = vc.GMMMap(r["weights"], r["means"], vc.expand_block_diag(r["covars"]))
    XT = np.asfortranarray(Z[:, :D].T)
    assert frame_relerr(vc.fvconvert(g, XT), vc.fvconvert(gd, XT)) < TOL
    Pd = vc.predict_proba(gd.px, XT)
    assert np.max(np.abs(vc.predict_proba(g.px, XT) - Pd)) < TOL
    clear = np.sort(Pd, axis=0)[-1] - np.sort(Pd, axis=0)[-2] > 1e-6
    assert clear.sum() > 0.9 * N and np.array_equal(vc.predict(g.px, XT)[clear], vc.predict(gd.px, XT)[clear])
    assert np.max(np.abs(g.slopes - np.stack([np.diag(gd.SyxSxxinv[:, :, m]) for m in range(M)], axis=1))) < 1e-12 * np.max(np.abs(g.slopes))
