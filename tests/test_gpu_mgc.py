"""GPU parity: sp2mc / mc2sp / mc2b (csrc/mgc.hip) against the numpy restatement (tests/mgc_restatement.py), host and
device entries, and the reference's conversion pipeline test/vc.jl:16,24-29 (envelope -> mel-cepstrum -> vc -> envelope)
and bin/vc.jl:76-87 (the trajectory leg) without WORLD.
Tolerances: per frame 1e-11 max(1, max_k |log sp_k|) for sp2mc, the same in the log domain for mc2sp; 1e-13 relative for
mc2b; 1e-8 in the log domain for the GMMMap pipeline, 1e-6 for the trajectory leg (the trajectory solver's own tolerance)."""
import ctypes as C

import numpy as np
import pytest

import mgc_restatement as mr
from conftest import julia_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vc():
    import voiceconversion_jl_amd as m
    assert m.device_count() >= 1
    return m


def log_spectrum(seed, K, T, scale=3.0):
    return scale * np.random.default_rng(seed).standard_normal((K, T))


def check_sp2mc(mc, ref, logsp):
    tol = 1e-11 * np.maximum(1.0, np.max(np.abs(logsp), axis=0))
    assert mc.shape == ref.shape
    assert np.all(np.max(np.abs(mc - ref), axis=0) <= tol), float(np.max(np.abs(mc - ref)))


def check_mc2sp(sp, ref):
    assert sp.shape == ref.shape
    lr = np.log(ref)
    tol = 1e-11 * np.maximum(1.0, np.max(np.abs(lr), axis=0))
    assert np.all(np.max(np.abs(np.log(sp) - lr), axis=0) <= tol), float(np.max(np.abs(np.log(sp) - lr)))


def device_matrix(a, ld):
    """(rows,T) numpy -> device tensor with leading dimension ld >= rows (unit stride along rows)."""
    import torch

    rows, T = a.shape
    buf = torch.full((max(T, 1), ld), float("nan"), dtype=torch.float64, device="cuda")
    v = buf[:T, :rows].t()
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


SP2MC_SHAPES = [(2, 1, 0.0), (3, 4, 0.41), (17, 25, -0.3), (257, 26, 0.58), (513, 41, 0.41), (513, 64, -0.3),
                (1025, 256, 0.58), (4097, 25, 0.41), (17, 256, 0.0), (257, 1, 0.41), (1025, 41, 0.0), (4097, 4, -0.3)]


@pytest.mark.parametrize("K,M1,alpha", SP2MC_SHAPES)
def test_sp2mc_host_and_device(vc, K, M1, alpha):
    T = 17
    logsp = log_spectrum(K + M1, K, T)
    sp = np.exp(logsp)
    ref = mr.sp2mc(sp, M1 - 1, alpha)
    check_sp2mc(vc.sp2mc(sp, M1 - 1, alpha), ref, logsp)
    d = vc.sp2mc(device_matrix(sp, K + 3), M1 - 1, alpha)
    assert d.is_cuda
    check_sp2mc(d.cpu().numpy(), ref, logsp)


MC2SP_SHAPES = [(2, 1, 0.0), (3, 4, 0.41), (32, 25, -0.3), (33, 26, 0.58), (512, 41, 0.41), (513, 64, -0.3),
                (1024, 41, 0.41), (1025, 41, 0.41), (2048, 256, 0.58), (2049, 26, 0.0), (8192, 41, -0.3), (8193, 1, 0.41),
                (4, 256, 0.41), (5, 25, 0.0)]


@pytest.mark.parametrize("fftlen,D,alpha", MC2SP_SHAPES)
def test_mc2sp_host_and_device(vc, fftlen, D, alpha):
    T = 17
    mc = mr.smooth_mc(fftlen + D, D, T, c0=-2.0)
    ref = mr.mc2sp(mc, alpha, fftlen)
    check_mc2sp(vc.mc2sp(mc, alpha, fftlen), ref)
    d = vc.mc2sp(device_matrix(mc, D + 5), alpha, fftlen)
    assert d.is_cuda
    check_mc2sp(d.cpu().numpy(), ref)


@pytest.mark.parametrize("D,alpha", [(1, 0.41), (4, -0.3), (25, 0.58), (26, 0.0), (41, 0.41), (64, -0.3), (256, 0.58)])
def test_mc2b_host_and_device(vc, D, alpha):
    mc = mr.smooth_mc(D, D, 33, scale=2.0)
    ref = mr.mc2b(mc, alpha)
    scale = np.max(np.abs(ref))
    assert np.max(np.abs(vc.mc2b(mc, alpha) - ref)) <= 1e-13 * scale
    d = vc.mc2b(device_matrix(mc, D + 2), alpha)
    assert np.max(np.abs(d.cpu().numpy() - ref)) <= 1e-13 * scale
    if alpha == 0.0:
        assert np.array_equal(vc.mc2b(mc, 0.0), mc)


@pytest.mark.parametrize("T", [0, 1, 15, 16, 17, 4099])
def test_frame_counts(vc, T):
    import torch

    K, order, alpha = 513, 40, 0.41
    logsp = log_spectrum(T, K, T)
    sp = np.exp(logsp)
    mc = vc.sp2mc(sp, order, alpha)
    assert mc.shape == (order + 1, T)
    if T == 0:
        assert vc.mc2sp(mc, alpha, 1024).shape == (K, 0) and vc.mc2b(mc, alpha).shape == (order + 1, 0)
        assert vc.sp2mc(torch.empty((0, K), dtype=torch.float64, device="cuda").t(), order, alpha).shape == (order + 1, 0)
        return
    check_sp2mc(mc, mr.sp2mc(sp, order, alpha), logsp)
    for fftlen in (1024, 1025):
        check_mc2sp(vc.mc2sp(mc, alpha, fftlen), mr.mc2sp(mc, alpha, fftlen))
    check_mc2sp(vc.mc2sp(device_matrix(mc, 48), alpha, 1025).cpu().numpy(), mr.mc2sp(mc, alpha, 1025))
    ref_b = mr.mc2b(mc, alpha)
    assert np.max(np.abs(vc.mc2b(mc, alpha) - ref_b)) <= 1e-13 * np.max(np.abs(ref_b))


def test_vectors_are_single_frames(vc):
    import torch

    sp = np.exp(log_spectrum(7, 513, 1))[:, 0]
    mc = vc.sp2mc(sp, 40, 0.41)
    assert mc.shape == (41,)
    check_sp2mc(mc[:, None], mr.sp2mc(sp[:, None], 40, 0.41), np.log(sp)[:, None])
    assert vc.mc2sp(mc, 0.41, 1025).shape == (513,)
    assert vc.mc2b(mc, 0.41).shape == (41,)
    d = vc.sp2mc(torch.from_numpy(sp).cuda(), 40, 0.41)
    assert d.shape == (41,) and d.is_cuda
    check_sp2mc(d.cpu().numpy()[:, None], mr.sp2mc(sp[:, None], 40, 0.41), np.log(sp)[:, None])


def test_exp_range_of_mc2sp(vc):
    # mc2sp's exp covers the whole range: large positive log spectra overflow to +inf as Julia's exp does
    mc = np.zeros((3, 3))
    mc[0] = [350.0, 354.0, -380.0]                         # log sp = 2 c0: 700 (finite), 708 (finite), -760 (0)
    sp = vc.mc2sp(mc, 0.0, 16)
    assert np.allclose(sp[:, 0], np.exp(700.0), rtol=1e-14) and np.allclose(sp[:, 1], np.exp(708.0), rtol=1e-14)
    assert np.all(sp[:, 2] == 0.0)
    mc[0] = [360.0, 0.0, np.nan]
    sp = vc.mc2sp(mc, 0.0, 16)
    assert np.all(np.isinf(sp[:, 0])) and np.all(sp[:, 1] == 1.0) and np.all(np.isnan(sp[:, 2]))


def joint_pipeline_inputs(joint_model, T, seed):
    w, mu, sig = joint_model
    rng = np.random.default_rng(seed)
    m = rng.integers(0, len(w), T)
    src = mu[m, :40].T + 0.05 * rng.standard_normal((40, T)) * 0.8 ** np.arange(40)[:, None]
    c0 = -4.0 + 0.5 * rng.standard_normal((1, T))
    mc = np.vstack([c0, src])
    return mr.mc2sp(mc, 0.41, 1024)                        # (513, T): the envelope cheaptrick would give at 1024


def test_reference_pipeline_test_vc_jl(vc, joint_model):
    """test/vc.jl:16,24-29: src = sp2mc(sp, 40, 0.41); converted = vc(GMMMap(model), src); mc2sp(converted, 0.41, 1025)."""
    import torch
    from oracle import c_oracle as co

    sp = joint_pipeline_inputs(joint_model, 300, 1)
    g = vc.GMMMap(*julia_model(*joint_model))
    ref_mc = mr.sp2mc(sp, 40, 0.41)
    ref_conv = co.GMMMap(*joint_model).vc(ref_mc.T).T
    ref = np.log(mr.mc2sp(ref_conv, 0.41, 1025))

    out = vc.mc2sp(vc.vc(g, vc.sp2mc(sp, 40, 0.41)), 0.41, 1025)          # host entries
    assert out.shape == (513, 300)
    assert np.max(np.abs(np.log(out) - ref)) <= 1e-8

    # the whole chain on device tensors: no host copy between the three steps
    T = sp.shape[1]
    dsp = torch.from_numpy(np.ascontiguousarray(sp.T)).cuda().t()
    dmc = vc.sp2mc(dsp, 40, 0.41)
    conv = torch.empty((T, 41), dtype=torch.float64, device="cuda").t()
    conv[0] = dmc[0]                                                         # row 1 passes through (src/common.jl:23)
    vc.fvconvert(g, dmc[1:], out=conv[1:])
    dout = vc.mc2sp(conv, 0.41, 1025)
    assert dout.is_cuda
    assert np.max(np.abs(np.log(dout.cpu().numpy()) - ref)) <= 1e-8


def test_reference_pipeline_trajectory_leg(vc):
    """bin/vc.jl:76-87: sp2mc, push_delta of the static rows on the device, TrajectoryGMMMap vc, mc2sp."""
    import torch
    from oracle import c_oracle as co
    from oracle import np_oracle as npo

    D, M, T = 24, 4, 120
    w, mu, sig = npo.synth_model(500 + D, 4 * D, M, lam_lo=1e-3)
    static = npo.sample_frames(77, w, mu, sig, T, 0, D)
    static = np.cumsum(static, axis=0) / np.sqrt(np.arange(1, T + 1))[:, None]
    mc = np.vstack([-3.0 + 0.1 * np.random.default_rng(5).standard_normal((1, T)), 0.3 * static.T])
    sp = mr.mc2sp(mc, 0.41, 512)

    ref_mc = mr.sp2mc(sp, D, 0.41)
    ref_fm = np.vstack([ref_mc[:1], npo.push_delta(ref_mc[1:].T).T])
    ref_conv = co.TrajectoryGMMMap(co.GMMMap(w, mu, sig)).vc(ref_fm.T, T).T
    ref = np.log(mr.mc2sp(ref_conv, 0.41, 511))

    t = vc.TrajectoryGMMMap(vc.GMMMap(*julia_model(w, mu, sig)), T)
    dmc = vc.sp2mc(torch.from_numpy(np.ascontiguousarray(sp.T)).cuda().t(), D, 0.41)
    dX = vc.push_delta(dmc[1:])
    fm = np.vstack([dmc[:1].cpu().numpy(), dX.cpu().numpy()])
    out = vc.mc2sp(vc.vc(t, fm), 0.41, 511)
    assert np.max(np.abs(np.log(out) - ref)) <= 1e-6              # the trajectory solver's tolerance (test_gpu_trajectory.py)


def test_errors(vc):
    from voiceconversion_jl_amd import _lib

    sp = np.exp(log_spectrum(9, 65, 20))
    for bad in (0.0, -1.0, np.nan, np.inf):
        s = sp.copy()
        s[30, 13] = bad
        with pytest.raises(vc.VCMIError, match="positive and finite"):
            vc.sp2mc(s, 20, 0.41)
    vc.sp2mc(sp, 20, 0.41)                                   # the flag is reset per call
    mc = mr.smooth_mc(1, 21, 4)
    for a in (1.0, -1.0, 1.5, np.nan):
        with pytest.raises(vc.VCMIError, match="alpha"):
            vc.sp2mc(sp, 20, a)
        with pytest.raises(vc.VCMIError, match="alpha"):
            vc.mc2sp(mc, a, 64)
        with pytest.raises(vc.VCMIError, match="alpha"):
            vc.mc2b(mc, a)
    for n in (1, 0, -4, 8194):
        with pytest.raises(vc.VCMIError, match="fftlen"):
            vc.mc2sp(mc, 0.41, n)
    with pytest.raises(vc.DimensionMismatch):
        vc.sp2mc(np.ones((1, 4)), 20, 0.41)                   # K < 2
    with pytest.raises(vc.DimensionMismatch):
        vc.sp2mc(np.ones((4098, 2)), 20, 0.41)
    with pytest.raises(vc.DimensionMismatch):
        vc.sp2mc(sp, 256, 0.41)                               # order + 1 > 256
    with pytest.raises(vc.DimensionMismatch):
        vc.mc2sp(np.zeros((257, 2)), 0.41, 64)
    L = _lib.lib
    out = np.empty((21, 20), order="F")
    dp = C.POINTER(C.c_double)
    assert L.vcmi_sp2mc(None, 65, 20, 20, 0.41, _lib.dptr(out)) == _lib.VCMI_ERR_ARG
    assert L.vcmi_sp2mc(_lib.dptr(np.asfortranarray(sp)), 65, 20, 20, 0.41, C.cast(None, dp)) == _lib.VCMI_ERR_ARG
    assert L.vcmi_mc2sp(None, 21, 4, 0.41, 64, _lib.dptr(out)) == _lib.VCMI_ERR_ARG
    assert L.vcmi_mc2b(None, 21, 4, 0.41, _lib.dptr(out)) == _lib.VCMI_ERR_ARG
    assert L.vcmi_sp2mc_dev(None, 65, 65, 20, 20, 0.41, None, 21, None) == _lib.VCMI_ERR_ARG
    assert L.vcmi_mc2sp_dev(None, 21, 21, 4, 0.41, 64, None, 33, None) == _lib.VCMI_ERR_ARG
    assert L.vcmi_mc2b_dev(None, 21, 21, 4, 0.41, None, 21, None) == _lib.VCMI_ERR_ARG
    assert "NULL" in _lib.last_error()
    assert L.vcmi_sp2mc(_lib.dptr(np.asfortranarray(sp)), 1, 20, 20, 0.41, _lib.dptr(out)) == _lib.VCMI_ERR_DIM


def test_repeat_calls_are_bit_identical(vc):
    sp = np.exp(log_spectrum(11, 513, 5000))
    a = vc.sp2mc(sp, 40, 0.41)
    b = vc.sp2mc(sp, 40, 0.41)
    assert np.array_equal(a, b)
    s1 = vc.mc2sp(a, 0.41, 1025)
    s2 = vc.mc2sp(a, 0.41, 1025)
    assert np.array_equal(s1, s2)
    assert np.array_equal(vc.mc2b(a, 0.41), vc.mc2b(a, 0.41))
