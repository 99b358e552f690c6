"""Longer QC-LDPC codes (lifting sizes 128 and 256: n = 3072, 6144), host side (no GPU): the committed tables, the
Z-parameterised restatement (tests/ldpc_ref_z.py) against the Z = 64 one, and that the longer code is worth having."""
import os
import sys

import numpy as np
import pytest

from tests import ldpc_ref as R64
from tests import ldpc_ref_z as RZ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = {"1/2": 12, "2/3": 8, "3/4": 6, "5/6": 4}


def table(rate, Z):
    from gf3_audio_modem_amd.ldpc import shift_table
    return shift_table(rate, Z)


@pytest.mark.parametrize("Z", [128, 256])
@pytest.mark.parametrize("rate", list(RATES))
def test_committed_table_properties(rate, Z):
    sh = table(rate, Z)
    assert sh.dtype == np.int16 and sh.shape == (RATES[rate], 24)
    # no 4-cycles mod Z, message-column degree >= 3, dual diagonal, H c^T = 0, shifts in [-1, Z)
    assert len(RZ.check_properties(sh, Z, seed=3, n_msg=16)) == 4
    assert sh.min() >= -1 and sh.max() < Z
    assert sh.max() >= 64                                  # the table uses what Z = 64 cannot express


@pytest.mark.parametrize("Z", [128, 256])
def test_committed_tables_are_the_generators(Z):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_qcldpc
    finally:
        sys.path.pop(0)
    tabs = make_qcldpc.generate(Z)
    for rate, sh in tabs.items():
        assert np.array_equal(sh, table(rate, Z)), rate
    assert open(make_qcldpc.out_path(Z)).read() == make_qcldpc.dumps(tabs, Z)
    assert open(make_qcldpc.out_path(64)).read() == make_qcldpc.dumps(make_qcldpc.generate(), 64)   # byte for byte


def test_shift_table_defaults_and_refusals():
    from gf3_audio_modem_amd.ldpc import shift_table
    assert np.array_equal(shift_table("1/2"), shift_table("1/2", 64)) and shift_table("1/2").max() < 64
    with pytest.raises(ValueError, match="Z=96"):
        shift_table("1/2", 96)
    with pytest.raises(ValueError, match="rate"):
        shift_table("7/8", 128)


@pytest.mark.parametrize("rate", list(RATES))
def test_restatement_with_z64_is_the_z64_restatement(rate):
    sh = table(rate, 64)
    k = (24 - sh.shape[0]) * 64
    rng = np.random.default_rng(13)
    msg = rng.integers(0, 2, size=(6, k), dtype=np.uint8)
    cw = R64.encode(sh, msg)
    assert np.array_equal(RZ.encode(sh, msg, 64), cw)
    assert np.array_equal(RZ.expand(sh, 64), R64.expand(sh))
    sig = np.linspace(0.3, 1.4, 6)[:, None]
    llr = ((1.0 - 2.0 * cw + rng.normal(size=cw.shape) * sig) * 2.0 / sig ** 2).astype(np.float32)
    llr[:, ::53] = 0.0                                     # zeros and exact ties
    llr[:, 3::71] = 1.25
    llr[:, 5::71] = -1.25
    assert np.array_equal(RZ.syndrome(sh, llr < 0, 64), R64.syndrome(sh, llr < 0))
    for it in (1, 10, 50):
        b0, a0, i0 = R64.decode(sh, llr, it)
        b1, a1, i1 = RZ.decode(sh, llr, it, 64)
        assert np.array_equal(b0, b1) and np.array_equal(i0, i1)
        assert np.array_equal(a0.view(np.int32), a1.view(np.int32))
    assert (i0 > 0).any() and (i0 < 0).any()


def test_wrap_is_mod_z_not_mod_64():
    """A circulant of shift s >= 64 at Z = 128 reaches the other half of the block; one wrapped mod 64 does not."""
    sh = np.array([[70, 0, -1], [-1, 127, 0]], dtype=np.int16)
    H = RZ.expand(sh, 128)
    assert H.shape == (256, 384) and H[0, 70] == 1 and H[60, 2] == 1 and H[128 + 1, 128] == 1
    assert (H.sum(axis=1) == 2).all()


# ---- that the longer code is worth having -----------------------------------------------------------------------
# Rate 1/2, BPSK/AWGN, 20 iterations, the same number of coded bits per lifting size (393 216), one seed per size.
# Swept with the restatement on a 0.25 dB grid of Eb/N0; failed codewords of 256 / 128 / 64 at Z = 64 / 128 / 256:
#   1.00 dB  149 / 91 / 50      1.25 dB  76 / 42 / 12      1.50 dB  19 / 7 / 0      1.75 dB  2 / 2 / 0      2.00 dB and above  0 / 0 / 0
FER_SEED = {64: 64, 128: 128, 256: 256}
FER_N_CW = {64: 256, 128: 128, 256: 64}
FER_POINT_DB = 1.5    # the lowest grid point at which all 64 Z = 256 codewords decode


def fer_run(Z, ebn0_db, max_iter=20):
    """Failed codewords (wrong message bits) of FER_N_CW[Z] rate-1/2 codewords at this Eb/N0."""
    sh = table("1/2", Z)
    n, k = 24 * Z, 12 * Z
    rng = np.random.default_rng(FER_SEED[Z])
    msg = rng.integers(0, 2, size=(FER_N_CW[Z], k), dtype=np.uint8)
    cw = RZ.encode(sh, msg, Z)
    sig2 = 1.0 / (2 * (k / n) * 10 ** (ebn0_db / 10))
    y = 1.0 - 2.0 * cw + rng.normal(0, np.sqrt(sig2), cw.shape)
    llr = (2 * y / sig2).astype(np.float32)
    bits, _, _ = RZ.decode(sh, llr, max_iter, Z)
    return int((bits != msg).any(axis=1).sum())


def test_longer_code_has_the_steeper_waterfall():
    assert fer_run(256, FER_POINT_DB) == 0
    assert fer_run(64, FER_POINT_DB) >= 1
