"""Inputs of the dataset front-end tests (tests/test_gpu_datasets_edges.py, tests/test_dataset_cases_host.py): mel-cepstrum-like
utterances whose kept / dropped frames are DICTATED through oracle/adversarial.frames_at_energy_threshold, so that the tests know
the kept pattern without asking the code under test.  Only numpy and the C oracle are used here."""
import numpy as np

ALPHA, FFTLEN, THRESHOLD = 0.41, 256, -14.0
# either side of the threshold of src/align.jl:49-51, from 1e-9 (1000 x what a 1e-12 relative error of mc2e moves log e by) to 0.5
TIGHT_GAPS = (1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3, 0.5, -0.5)
MIN_GAP = 5e-10


def mcep(rng, T, D):
    """decaying coefficients, c0 spread over the range of speech and silence"""
    mc = rng.standard_normal((T, D)) * np.exp(-0.3 * np.arange(D)) * 0.3
    mc[:, 0] = rng.uniform(-9.0, 1.0, T)
    return mc


def warped_copy(rng, src, T):
    """a target that DTW aligns unambiguously: frames of src in order, with repeats / skips, plus a little noise"""
    S, D = src.shape
    idx = np.clip(np.sort(rng.integers(0, S, T)), 0, S - 1)
    return src[idx] + 0.01 * rng.standard_normal((T, D))


def dictated(rng, keep, D, alpha=ALPHA, fftlen=FFTLEN, threshold=THRESHOLD, gap=0.5):
    """(len(keep), D) utterance whose frame i lies `gap` above the threshold where keep[i], `gap` below it elsewhere"""
    from oracle import adversarial as adv
    keep = np.asarray(keep, dtype=bool)
    mc, got = adv.frames_at_energy_threshold(mcep(rng, len(keep), D), alpha, fftlen, threshold, np.where(keep, gap, -gap))
    assert np.array_equal(got > 0, keep) and np.all(np.abs(got) > 0.9 * gap)
    return mc


def keep_with_count(rng, S, k):
    keep = np.zeros(S, dtype=bool)
    keep[rng.choice(S, k, replace=False)] = True
    return keep


def threshold_case(S=320, T=300, D=25, seed=5):
    """source frames cycling through TIGHT_GAPS either side of the threshold, and a warped copy as target.
    Returns (src (S,D), tgt (T,D), requested gaps, achieved gaps)."""
    from oracle import adversarial as adv
    rng = np.random.default_rng(seed)
    want = np.resize(np.array(TIGHT_GAPS), S)
    src, got = adv.frames_at_energy_threshold(mcep(rng, S, D), ALPHA, FFTLEN, THRESHOLD, want)
    return src, warped_copy(rng, src, T), want, got


def seam_patterns(rng, S):
    """the keep patterns that put a kept / dropped boundary on every seam of the compaction: the 64-lane ballot, the
    256-frame iteration and both ends"""
    only = lambda *ix: np.isin(np.arange(S), ix)
    pats = [("all", np.ones(S, bool)), ("none", np.zeros(S, bool)), ("first", only(0)), ("last", only(S - 1))]
    if S > 64:
        pats.append(("63,64", only(63, 64)))
    if S > 256:
        pats.append(("255,256", only(255, 256)))
    pats.append(("alternating", np.arange(S) % 2 == 1))
    pats.append(("random half", keep_with_count(rng, S, S // 2)))
    return pats
