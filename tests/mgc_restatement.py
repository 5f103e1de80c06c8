"""numpy restatement of MelGeneralizedCepstrums' sp2mc, mc2sp and mc2b as the library defines them (test helper, not a
test module), written literally: the SPTK freqt recursion, numpy's irfft / rfft, the symmetric vector -- not the folded
matrices the library builds.  Matrices are (rows, T), one frame per column, as in Julia."""
import numpy as np


def freqt(c, m2, a):
    """SPTK freqt: frequency warping of the cepstra in the columns of c ((m1+1, T) or a vector) to m2+1 coefficients."""
    c = np.asarray(c, dtype=np.float64)
    vec = c.ndim == 1
    c2 = c.reshape(c.shape[0], -1)
    m1, b = c2.shape[0] - 1, 1.0 - a * a
    g = np.zeros((m2 + 1, c2.shape[1]))
    for i in range(m1, -1, -1):
        d = g.copy()
        g[0] = c2[i] + a * d[0]
        if m2 >= 1:
            g[1] = b * d[0] + a * d[1]
        for j in range(2, m2 + 1):
            g[j] = d[j - 1] + a * (d[j] - g[j - 1])
    return g[:, 0] if vec else g


def sp2mc(sp, order, alpha):
    """sp (K,T) power spectra -> (order+1, T): c = irfft(log sp, 2(K-1)), c[0] /= 2, freqt over ALL 2(K-1) entries."""
    sp = np.asarray(sp, dtype=np.float64)
    K = sp.shape[0]
    c = np.fft.irfft(np.log(sp), 2 * (K - 1), axis=0)
    c[0] /= 2
    return freqt(c, order, alpha)


def mc2sp(mc, alpha, fftlen):
    """mc (D,T) -> (fftlen//2+1, T): c = freqt(mc, fftlen//2, -alpha), c[0] *= 2, s[0..L] = c, s[fftlen-i] = c[i],
    exp(real(rfft(s)))."""
    mc = np.asarray(mc, dtype=np.float64)
    L = fftlen // 2
    c = freqt(mc, L, -alpha)
    c[0] *= 2
    s = np.zeros((fftlen,) + c.shape[1:])
    s[:L + 1] = c
    for i in range(1, L + 1):
        s[fftlen - i] = c[i]
    return np.exp(np.fft.rfft(s, axis=0).real)


def mc2b(mc, alpha):
    """b[D-1] = mc[D-1], b[i] = mc[i] - alpha b[i+1]."""
    mc = np.asarray(mc, dtype=np.float64)
    b = np.empty_like(mc)
    b[-1] = mc[-1]
    for i in range(mc.shape[0] - 2, -1, -1):
        b[i] = mc[i] - alpha * b[i + 1]
    return b


def log_sp_frequency_domain(mc, alpha, fftlen):
    """log of the power spectrum a mel-cepstrum describes, evaluated directly on the unit circle (no freqt, no FFT):
    2 Re sum_m mc_m z~^-m at z = exp(j 2 pi k / fftlen), z~^-1 = (z^-1 - alpha) / (1 - alpha z^-1).  (fftlen//2+1, T)"""
    mc = np.atleast_2d(np.asarray(mc, dtype=np.float64).T).T
    k = np.arange(fftlen // 2 + 1)
    zi = np.exp(-2j * np.pi * k / fftlen)
    zt = (zi - alpha) / (1.0 - alpha * zi)
    powers = np.ones((mc.shape[0], len(k)), dtype=np.complex128)
    for m in range(1, mc.shape[0]):
        powers[m] = powers[m - 1] * zt
    return 2.0 * (powers.T @ mc.astype(np.complex128)).real


def smooth_mc(seed, D, T, c0=0.0, scale=1.0, decay=0.7):
    """Mel-cepstra with coefficients that fall off geometrically (a smooth envelope), row 0 = c0 + noise."""
    rng = np.random.default_rng(seed)
    mc = scale * rng.standard_normal((D, T)) * decay ** np.arange(D)[:, None]
    mc[0] += c0
    return mc
