"""GPU: TrajectoryGVGMMMap for static dimensions above 48 (2D > 96: traj_gvw_kernel, csrc/traj_gv.hip) -- every entry that
follows the converter, against the C oracle's fvconvert_gv.
Models, utterances and GV statistics are built as in test_gpu_gv.py; the tolerance is that file's 1e-6 relative, for its reason
(the two sides start the ascent from different direct solvers, cond(P) ~ 1e6; the C oracle and the literal numpy restatement
of the ascent agree to 3e-13 at these shapes).  Two library paths that run the same kernels on the same bytes are compared bit
for bit."""
import functools

import numpy as np
import pytest

import call_history as ch
import gv_restatement as gr
from conftest import julia_model, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-6
ALPHA = 1.0e-5
# kGvwPermLds (csrc/traj_gv.hip): slots of the frame permutation traj_gvw_kernel keeps in LDS; an utterance of T frames over M
# mixtures can need (ceil(T / 16) + M) * 16 of them, beyond that the permutation lives in the workspace
PERM_LDS_SLOTS = 1024


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def _gv_stats(rng, Y):
    """GV mean slightly above the converted track's variance, and a dense SPD GV covariance (the recipe of test_gpu_gv.py)."""
    D = Y.shape[1]
    muv = Y.var(axis=0, ddof=1) * 1.3
    A = rng.standard_normal((D, D))
    return muv, A @ A.T / D * np.mean(muv) ** 2 * 0.1 + np.diag(muv ** 2 * 0.05)


def _utterances(npo, rng, w, mu, sig, D, Ts):
    Xs = []
    for T in Ts:
        static = npo.sample_frames(int(rng.integers(1 << 30)), w, mu, sig, T, 0, D)
        static = np.cumsum(static, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
        Xs.append(npo.push_delta(static))
    return Xs


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _model(D, M, seed=None):
    from oracle import np_oracle as npo
    return npo.synth_model(600 + D if seed is None else seed, 4 * D, M, lam_lo=1e-3)


@functools.lru_cache(maxsize=None)
def _case(D, M, Ts, rng_seed=None, model_seed=None):
    """Model, utterances (T, 2D), GV statistics from the oracle's plain trajectory of the first utterance, that trajectory and
    its mixture sequence -- computed once, shared read-only."""
    from oracle import c_oracle as co, np_oracle as npo
    w, mu, sig = _model(D, M, model_seed)
    ref = co.TrajectoryGMMMap(co.GMMMap(w, mu, sig))
    rng = np.random.default_rng(D if rng_seed is None else rng_seed)
    Xs = [_frozen(x) for x in _utterances(npo, rng, w, mu, sig, D, Ts)]
    y0, mhat0, _ = ref.fvconvert(Xs[0])
    muv, Sv = _gv_stats(rng, y0 if y0.shape[0] > 2 else np.vstack([y0, y0 + 1.0]))
    return dict(model=(w, mu, sig), ref=ref, Xs=Xs, y0=_frozen(y0), mhat0=_frozen(np.asarray(mhat0).ravel()), muv=_frozen(muv),
                Sv=_frozen(Sv))


def _mixtures_in_a_run(mhat, run=16):
    """most distinct mixtures among `run` consecutive frames"""
    return max(len(set(mhat[t:t + run].tolist())) for t in range(max(1, len(mhat) - run + 1)))


def _make(vc, c, L):
    t = vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*c["model"])), L)
    return t, vc.TrajectoryGVGMMMap(t, c["muv"], c["Sv"])


# D = 130: seed 600 + D with M = 3 puts every frame in one mixture; M = 6 with the seed below does not (asserted in the test)
ORACLE_CASES = [(49, 5, (70, 33, 2), 20, None), (52, 4, (300, 17), 20, None), (66, 6, (40, 9), 25, None), (130, 6, (37,), 10, 731)]


@pytest.mark.parametrize("D,M,Ts,epochs,model_seed", ORACLE_CASES)
def test_vs_oracle_batch(vc, D, M, Ts, epochs, model_seed):
    """D = 49: the first dimension above the old limit -- seven row tiles, 2D = 98 = 24 * 4 + 2 (a partial last k-step, a last
    row tile with two live rows), T = 2 with both stencil neighbours missing; D = 52: whole k-steps, a long and a short
    utterance; D = 66: the fallback solver with its window in HBM; D = 130: 2D = 260, seventeen row tiles (two passes over the
    rows) and five k chunks.  The reference's default alpha."""
    _vs_oracle_batch(vc, D, M, Ts, epochs, model_seed, ALPHA, 1.0)


# the shapes of ORACLE_CASES without the two-frame utterance, which diverges at the step-visible values
STEP_VISIBLE_CASES = [(49, 5, (70, 33), 20, None), (52, 4, (300, 17), 20, None), (66, 6, (40, 9), 25, None), (130, 6, (37,), 10, 731)]


@pytest.mark.parametrize("D,M,Ts,epochs,model_seed", STEP_VISIBLE_CASES)
def test_vs_oracle_batch_step_visible(vc, D, M, Ts, epochs, model_seed):
    """the same shapes at the step size and GV covariance scale where the ascent moves y by 1e-2 of its size and both gradient
    terms count (gv_restatement.ORACLE_ALPHA, ORACLE_COV_SCALE).  Besides y, the INCREMENT y_epochs - y_0 is compared, each
    side against its own epochs = 0, relative to max |increment|, with the bar of gv_restatement.increment_bar (derived there
    from the solvers' parity bar, the eq. (58) scale and |A - I| <= 2; see tests/test_gpu_gv.py), not taken from a run of the
    kernel."""
    _vs_oracle_batch(vc, D, M, Ts, epochs, model_seed, gr.ORACLE_ALPHA, gr.ORACLE_COV_SCALE)


def _vs_oracle_batch(vc, D, M, Ts, epochs, model_seed, alpha, cov_scale):
    c = _case(D, M, Ts, None, model_seed)
    ref, Xs, muv, Sv = c["ref"], c["Xs"], c["muv"], c["Sv"] * cov_scale
    assert _mixtures_in_a_run(c["mhat0"]) >= 2, "the generator no longer mixes mixtures inside 16 frames"
    t = vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(*c["model"])), max(Ts))
    tgv = vc.TrajectoryGVGMMMap(t, muv, Sv)
    got = tgv.fvconvert_batch([x.T for x in Xs], epochs=epochs, alpha=alpha)
    for x, y in zip(Xs, got):
        want = ref.fvconvert_gv(x, muv, Sv, epochs, alpha)
        e = relerr(y, want.T)
        print(f"GV D={D} M={M} T={x.shape[0]} epochs={epochs} alpha={alpha:g}: vs oracle {e:.2e}")
        assert y.shape == (D, x.shape[0]) and e < TOL, x.shape
    if alpha != ALPHA:
        got0 = tgv.fvconvert_batch([x.T for x in Xs], epochs=0, alpha=alpha)
        missed = []
        for x, y, y0 in zip(Xs, got, got0):
            want, want0 = ref.fvconvert_gv(x, muv, Sv, epochs, alpha), ref.fvconvert_gv(x, muv, Sv, 0, alpha)
            inc, inc_ref = y.T - y0.T, want - want0
            bar, cond = gr.increment_bar(c["model"], x, want, want0, ref.fvconvert(x)[0], inc_ref, muv)
            e = float(np.max(np.abs(inc - inc_ref)) / np.max(np.abs(inc_ref)))
            print(f"GVINC D={D} T={x.shape[0]} epochs={epochs}: increment {np.max(np.abs(inc_ref)) / np.max(np.abs(want)):.2e} of max|y|, "
                  f"vs oracle {e:.2e} of it, bar {bar:.2e} (cond {cond:.3g})")
            assert np.max(np.abs(inc_ref)) > 1e-3 * np.max(np.abs(want)), x.shape
            if not e <= bar:
                missed.append((x.shape[0], e, bar))
        assert not missed, f"increment vs oracle beyond the bar (T, error, bar): {missed}"
    moved = relerr(got[0], c["y0"].T)
    print(f"   ascent vs the plain trajectory: {moved:.2e}")
    assert moved > 1e-3                                   # the ascent moved the trajectory
    # epochs = 0 is the eq. (58) initialisation alone = VarianceScaling(mu^v) of the plain trajectory
    init = vc.fvconvert(tgv, Xs[0].T, epochs=0)
    assert relerr(init, vc.fvpostf(vc.VarianceScaling(muv), vc.fvconvert(t, Xs[0].T))) < 1e-12
    with pytest.raises(vc.DimensionMismatch):
        tgv.fvconvert_batch([Xs[0][:1].T])                # a one-frame trajectory has no variance


def test_batch_equals_single_call(vc):
    """600 ragged utterances, more than compute units: every workgroup runs several one after the other; each result equals the
    single-utterance call bit for bit"""
    from oracle import np_oracle as npo
    D, M = 49, 4
    w, mu, sig = _model(D, M)
    rng = np.random.default_rng(8)
    Ts = [int(v) for v in rng.integers(2, 41, size=600)]
    Xs = _utterances(npo, rng, w, mu, sig, D, Ts)
    c = _case(D, M, (40,))
    _, tgv = _make(vc, c, 40)
    got = tgv.fvconvert_batch([x.T for x in Xs], epochs=7, alpha=ALPHA)
    for i in list(range(0, 600, 41)) + [599]:
        assert np.array_equal(vc.fvconvert(tgv, Xs[i].T, epochs=7, alpha=ALPHA), got[i]), i
        assert np.all(np.isfinite(got[i]))


def test_long_utterance(vc):
    """traj_gvw_kernel keeps the frame permutation in LDS while (ceil(T / 16) + M) * 16 <= 1024 slots (kGvwPermLds); T = 1100
    with M = 3 needs 1152: the permutation lives in the workspace behind V and r"""
    D, M, T = 49, 3, 1100
    assert ((T + 15) // 16 + M) * 16 > PERM_LDS_SLOTS
    c = _case(D, M, (T,))
    _, tgv = _make(vc, c, T)
    got = vc.fvconvert(tgv, c["Xs"][0].T, epochs=3, alpha=ALPHA)
    e = relerr(got, c["ref"].fvconvert_gv(c["Xs"][0], c["muv"], c["Sv"], 3, ALPHA).T)
    print(f"GV D={D} T={T}: vs oracle {e:.2e}")
    assert e < TOL


@functools.lru_cache(maxsize=None)
def _vc_case():
    """D = 49, M = 4: static features of three utterances (70, 31 and 32 frames), their whole-utterance deltas, GV statistics"""
    from oracle import c_oracle as co, np_oracle as npo
    D, M = 49, 4
    w, mu, sig = _model(D, M, 77)
    ref = co.TrajectoryGMMMap(co.GMMMap(w, mu, sig))
    rng = np.random.default_rng(3)
    out = dict(model=(w, mu, sig), ref=ref, D=D)
    for T in (70, 31, 32):
        st = npo.sample_frames(int(rng.integers(1 << 30)), w, mu, sig, T, 0, D)
        st = np.cumsum(st, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
        X = co.push_delta(st)
        power = np.linspace(0, 1, T)
        out[T] = dict(X=_frozen(X), power=_frozen(power), fm_static=_frozen(np.asfortranarray(np.vstack([power[None], st.T]))),
                      fm=_frozen(np.asfortranarray(np.vstack([power[None], X.T]))))
    muv, Sv = _gv_stats(rng, ref.fvconvert(out[70]["X"])[0])
    out["muv"], out["Sv"] = _frozen(muv), _frozen(Sv)
    return out


def test_vc_family(vc):
    """vc(tgv, fm) in chunks of len(tgv) = 30 at the wide dimension: the (2D+1,T) matrix per chunk against the oracle, static
    input with the post-filter from a host matrix and from a device tensor, and vc_batch against vc on fresh converters"""
    import torch
    c = _vc_case()
    D, L, T = c["D"], 30, 70
    ref, muv, Sv, u = c["ref"], c["muv"], c["Sv"], c[70]

    def make():
        return _make(vc, c, L)[1]

    tgv = make()
    out = vc.vc(tgv, u["fm"])
    assert out.shape == (D + 1, T) and np.array_equal(out[0], u["power"])
    for b in range(0, T, L):
        want = ref.fvconvert_gv(u["X"][b:b + L], muv, Sv, 100, ALPHA)
        e = relerr(out[1:, b:b + L], want.T)
        print(f"GV vc D={D}, chunk at {b}: vs oracle {e:.2e}")
        assert e < TOL
    vs = vc.VarianceScaling(np.random.default_rng(2).uniform(0.5, 2.0, D))
    host = vc.vc(make(), u["fm_static"], postfilter=vs, delta=True)
    assert host.shape == (D + 1, T) and np.array_equal(host[0], u["power"])
    assert np.allclose(host[1:].var(axis=1, ddof=1), vs.sigma2, rtol=1e-9)
    dev = vc.vc(make(), torch.from_numpy(np.array(u["fm_static"].T, order="C")).cuda().t(), postfilter=vs, delta=True)
    assert dev.is_cuda and ch.same_bits(dev.cpu().numpy(), host)
    # THE RULE of vc_batch (include/vcmi.h): each result is what vc on a fresh converter returns for that utterance
    fms = [c[70]["fm_static"], c[32]["fm_static"]]
    tb = make()
    got = vc.vc_batch(tb, fms, postfilter=vs, delta=True)
    assert len(tb) == L
    for fm, g in zip(fms, got):
        assert ch.same_bits(np.asarray(g), vc.vc(make(), fm, postfilter=vs, delta=True))
    # ... also where vc refuses: 31 frames at L = 30 leave a chunk of one frame, which has no variance -- vc on a fresh converter
    # raises DimensionMismatch before anything runs, and so does vc_batch for the whole list (include/vcmi.h)
    t1 = make()
    with pytest.raises(vc.DimensionMismatch):
        vc.vc(t1, c[31]["fm_static"], postfilter=vs, delta=True)
    with pytest.raises(vc.DimensionMismatch):
        vc.vc_batch(tb, [c[70]["fm_static"], c[31]["fm_static"]], postfilter=vs, delta=True)
    assert len(t1) == L and len(tb) == L


def test_call_history(vc):
    """a wide GV conversion after a narrow one (D = 12: traj_gv2_kernel, another workspace shape on the thread) and after a plain
    trajectory conversion gives the bits of a fresh thread with fresh handles; twice on one handle gives the same bits twice"""
    wide = _case(49, 5, (70, 33, 2))
    narrow = _case(12, 4, (50, 17))
    X = wide["Xs"][0].T

    def convert_fresh():
        return vc.fvconvert(_make(vc, wide, 70)[1], X, epochs=20, alpha=ALPHA)

    want = ch.to_numpy(ch.fresh(convert_fresh))
    tn, tgn = _make(vc, narrow, 50)
    tw, tgw = _make(vc, wide, 70)
    steps = ch.play([("narrow_gv", lambda: vc.fvconvert(tgn, narrow["Xs"][0].T, epochs=20, alpha=ALPHA)),
                     ("wide_gv_1", lambda: vc.fvconvert(tgw, X, epochs=20, alpha=ALPHA)),
                     ("wide_plain", lambda: vc.fvconvert(tw, wide["Xs"][1].T)),
                     ("wide_gv_other", lambda: vc.fvconvert(tgw, wide["Xs"][1].T, epochs=20, alpha=ALPHA)),
                     ("wide_gv_2", lambda: vc.fvconvert(tgw, X, epochs=20, alpha=ALPHA))])
    assert ch.same_bits(steps["wide_gv_1"], want) and ch.same_bits(steps["wide_gv_2"], want)
    assert relerr(steps["wide_gv_1"], wide["ref"].fvconvert_gv(wide["Xs"][0], wide["muv"], wide["Sv"], 20, ALPHA).T) < TOL


def test_em_is_still_refused(vc):
    """a wide GV converter over a trajectory handle with em_iters > 0 raises before anything runs; back at 0 it converts to the
    bits it gave before"""
    c = _case(49, 5, (70, 33, 2))
    t, tgv = _make(vc, c, 70)
    X = c["Xs"][0].T
    before = vc.fvconvert(tgv, X, epochs=20, alpha=ALPHA)
    t.em_iters = 1
    with pytest.raises(vc.VCMIError):
        vc.fvconvert(tgv, c["Xs"][1].T, epochs=20, alpha=ALPHA)
    t.em_iters = 0
    assert ch.same_bits(vc.fvconvert(tgv, X, epochs=20, alpha=ALPHA), before)
