"""What the GPU tests of the joint detectors (tests/test_mimo_gpu.py, tests/test_stbc_gpu.py, tests/test_joint_noise_gpu.py)
hold a call's LLRs to, stated once."""
import numpy as np


def held_to_the_restatement(part, ref, pair, const_bits, clear_share=0.99):
    """LLRs `part` against the restatement's `ref` at rtol 1e-6 and 1e-9 of the largest, and their signs against the bits
    of its joint argmin `pair` wherever the restated LLR is clear of that floor.  clear_share: the share of the cells that
    must be clear, each test's own figure from before the three copies became this function -- 0.99 for the unweighted
    detectors, 0.95 for the weighted ones of tests/test_joint_noise_gpu.py, whose inputs switch branches off."""
    assert part.shape == ref.shape
    atol = 1e-9 * np.abs(ref).max()
    np.testing.assert_allclose(part, ref, rtol=1e-6, atol=atol)
    clear = np.abs(ref) > atol
    assert clear.mean() > clear_share
    lab = np.asarray(const_bits)[pair].astype(bool)         # [..., mu]: the bits of the joint argmin
    assert np.array_equal((part < 0)[clear], lab[clear])
