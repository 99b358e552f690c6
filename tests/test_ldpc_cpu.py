"""QC-LDPC coding, host side (no GPU): the committed code tables, the NumPy restatement the GPU kernels are held to
(tests/ldpc_ref.py), and the façade's handling of the "QCLDPC-*" encodings."""
import os
import sys

import numpy as np
import pytest

from tests import ldpc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = {"1/2": (12, 768), "2/3": (8, 1024), "3/4": (6, 1152), "5/6": (4, 1280)}


def table(rate):
    from gf3_audio_modem_amd.ldpc import shift_table
    return shift_table(rate)


@pytest.mark.parametrize("rate", list(RATES))
def test_committed_table_properties(rate):
    sh = table(rate)
    mb, k = RATES[rate]
    assert sh.dtype == np.int16 and sh.shape == (mb, 24)
    lines = R.check_properties(sh, seed=3, n_msg=16)       # no 4-cycles, column degrees >= 3, dual diagonal, H c^T = 0
    assert len(lines) == 4
    assert (24 - mb) * 64 == k


def test_committed_tables_are_the_generators():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_qcldpc
    finally:
        sys.path.pop(0)
    for rate, sh in make_qcldpc.generate().items():
        assert np.array_equal(sh, table(rate)), rate


def test_dual_diagonal_rejects_other_parity_parts():
    sh = table("3/4").copy()
    assert R.dual_diagonal(sh) == (1, 3)
    sh[2, 18] = 5                                         # a third block in the first parity column
    assert R.dual_diagonal(sh) is None
    sh = table("3/4").copy()
    sh[3, 20] = 7                                         # a bidiagonal block with a non-zero shift
    assert R.dual_diagonal(sh) is None


def test_encoder_is_systematic_and_in_the_null_space():
    rng = np.random.default_rng(11)
    for rate, (mb, k) in RATES.items():
        sh = table(rate)
        msg = rng.integers(0, 2, size=(5, k), dtype=np.uint8)
        cw = R.encode(sh, msg)
        assert cw.shape == (5, 1536) and np.array_equal(cw[:, :k], msg)
        assert not R.syndrome(sh, cw).any()
        assert not R.syndrome(sh, R.encode(sh, np.zeros((1, k), np.uint8))).any()


def test_restatement_corrects_planted_errors():
    sh = table("1/2")
    rng = np.random.default_rng(5)
    msg = rng.integers(0, 2, size=(3, 768), dtype=np.uint8)
    cw = R.encode(sh, msg)
    llr = np.where(cw == 0, 4.0, -4.0).astype(np.float32)
    for b in range(3):                                    # 40 hard errors per codeword, with weaker magnitudes
        pos = rng.choice(1536, size=40, replace=False)
        llr[b, pos] = -0.5 * llr[b, pos]
    assert ((llr < 0) != cw).sum(axis=1).min() == 40
    bits, app, its = R.decode(sh, llr, 50)
    assert np.array_equal(bits, msg)
    assert np.array_equal((app < 0).astype(np.uint8), cw)
    assert (its > 0).all() and (its <= 50).all()


def test_restatement_stops_at_once_on_a_clean_codeword_and_reports_failure():
    sh = table("2/3")
    cw = R.encode(sh, np.random.default_rng(1).integers(0, 2, size=(1, 1024), dtype=np.uint8))
    llr = np.where(cw == 0, 1.0, -1.0).astype(np.float32)
    _, _, its = R.decode(sh, llr, 10)
    assert its.tolist() == [1]
    noise = np.random.default_rng(2).normal(0, 3.0, size=llr.shape).astype(np.float32)
    _, _, its = R.decode(sh, noise, 3)                    # pure noise: no codeword within 3 iterations
    assert its.tolist() == [-3]


# Eb/N0 (dB) per rate and the frame error rate of 100 codewords there; measured with the restatement (seed 7):
# 0 frame errors at each point (0.105 / 0.02 / 0.02 / 0.05 at 0.5 dB less), every frame with raw bit errors.
FER_POINTS = {"1/2": 2.0, "2/3": 3.0, "3/4": 3.5, "5/6": 4.0}


@pytest.mark.parametrize("rate", list(FER_POINTS))
def test_restatement_fer_on_bpsk_awgn(rate):
    sh = table(rate)
    k = RATES[rate][1]
    rng = np.random.default_rng(7)
    msg = rng.integers(0, 2, size=(100, k), dtype=np.uint8)
    cw = R.encode(sh, msg)
    sig2 = 1.0 / (2 * (k / 1536) * 10 ** (FER_POINTS[rate] / 10))
    y = 1.0 - 2.0 * cw + rng.normal(0, np.sqrt(sig2), cw.shape)     # (one QPSK axis = BPSK)
    llr = (2 * y / sig2).astype(np.float32)
    assert ((llr < 0) != cw).any(axis=1).all()
    bits, _, its = R.decode(sh, llr, 20)
    fer = (bits != msg).any(axis=1).mean()
    assert fer <= 0.02, fer
    assert (its > 0).mean() >= 0.98


def test_restatement_is_invariant_to_a_global_scale():
    sh = table("3/4")
    rng = np.random.default_rng(9)
    cw = R.encode(sh, rng.integers(0, 2, size=(8, 1152), dtype=np.uint8))
    llr = ((1 - 2.0 * cw) * 2.0 + rng.normal(0, 1.6, cw.shape)).astype(np.float32)
    llr[:, ::97] = 0.0                                    # zeros and exact ties
    llr[:, 5::89] = 0.75
    llr[:, 7::89] = -0.75
    for it in (1, 10, 50):
        b1, a1, i1 = R.decode(sh, llr, it)
        b4, a4, i4 = R.decode(sh, llr * np.float32(4.0), it)
        assert np.array_equal(b1, b4) and np.array_equal(i1, i4)
        assert np.array_equal(a4, a1 * np.float32(4.0))


# ---- façade (host-side plumbing: the GPU encoder is replaced by the restatement) -----------------------------------
class _HostCode:
    def __init__(self, rate):
        self.sh = table(rate)
        self.n, self.k = 1536, (24 - self.sh.shape[0]) * 64

    def encode(self, msg):
        import torch
        m = np.asarray(msg).reshape(-1, self.k)
        return torch.from_numpy(R.encode(self.sh, m))


@pytest.mark.parametrize("enc", ["QCLDPC-1/2", "QCLDPC-2/3", "QCLDPC-3/4", "QCLDPC-5/6"])
def test_facade_encode_and_sp_shapes(enc, monkeypatch):
    from gf3_audio_modem_amd import OFDM
    monkeypatch.setattr(OFDM, "_qcldpc_code", lambda rate, device=None: _HostCode(rate))
    tx = OFDM.transmitter("A2", encoding=enc)
    assert tx._qcldpc_rate() == enc.split("-")[1]
    code = _HostCode(tx._qcldpc_rate())
    payload = np.random.default_rng(3).integers(0, 2, size=5000)
    np.random.seed(4)
    out = tx.encode(payload)
    per_packet = tx.packet_length * tx.data_bits_per_symbol
    n_cw = -(-len(payload) // code.k)
    assert len(out) % per_packet == 0 and len(out) >= n_cw * code.n
    msg = np.concatenate([payload, np.zeros(n_cw * code.k - len(payload), dtype=payload.dtype)]).reshape(n_cw, code.k)
    assert np.array_equal(out[: n_cw * code.n], R.encode(code.sh, msg).reshape(-1))
    np.random.seed(4)                                     # the fill is the one legacy-RNG coin-flip draw
    assert np.array_equal(out[n_cw * code.n:], np.random.binomial(n=1, p=0.5, size=(len(out) - n_cw * code.n,)))
    sp = tx.SP(out)
    assert sp.shape == (len(out) // (tx.data_carriers_per_symbol * tx.mu), tx.data_carriers_per_symbol, tx.mu)


def test_facade_ldpc_encoding_unchanged():
    from gf3_audio_modem_amd.OFDM import receiver, transmitter
    with pytest.raises(NotImplementedError, match="LDPC encoding is out of scope"):
        transmitter("A2", encoding="LDPC").encode(np.zeros(10, dtype=int))
    with pytest.raises(NotImplementedError, match="LDPC decoding is out of scope"):
        receiver("A2", encoding="LDPC").decode(np.zeros(10, dtype=int))
    assert transmitter("A2", encoding="LDPC")._qcldpc_rate() is None
