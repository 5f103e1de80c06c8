"""CPU: the inputs that tests/test_gpu_datasets_edges.py places on the silence threshold are what they claim to be -- checked
with the C oracle alone, so that the GPU tests' preconditions are known to hold before a device is involved."""
import numpy as np

import dataset_cases as dc


def test_frames_land_on_the_requested_side_of_the_threshold():
    """c0 += a adds exactly 2a to log mc2e, so one step reaches the requested gap to a few ulp of log e ~ 14: every achieved gap
    has the requested sign and |gap| >= 5e-10, and the oracle's align_mcep keeps exactly the frames with a positive gap."""
    from oracle import c_oracle as co
    src, tgt, want, got = dc.threshold_case()
    assert np.array_equal(np.sign(got), np.sign(want))
    assert np.all(np.abs(got) >= dc.MIN_GAP)
    assert np.max(np.abs(got - want)) < 1e-13
    s_ref, t_ref = co.align_mcep(src, tgt, dc.ALPHA, dc.FFTLEN, dc.THRESHOLD)
    assert len(s_ref) == int((want > 0).sum()) == len(src) // 2
    assert np.array_equal(s_ref, src[want > 0])


def test_dictated_patterns_are_the_oracles_decision():
    from oracle import c_oracle as co
    rng = np.random.default_rng(3)
    for S in (63, 257):
        for name, keep in dc.seam_patterns(rng, S):
            mc = dc.dictated(rng, keep, 25)
            assert np.array_equal(np.log(co.mc2e(mc, dc.ALPHA, dc.FFTLEN)) > dc.THRESHOLD, keep), (S, name)
