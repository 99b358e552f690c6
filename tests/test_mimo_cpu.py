"""2 x 2 spatial multiplexing, host side (no GPU): the declared interface, the façade's refusals, the cover identity of the
NumPy restatement (tests/mimo_ref.py), the scenario of DESIGN §12 -- a 2 x 2 channel of 40-tap FIRs with speaker 1 six
samples early at one microphone and five late at the other -- noiseless and in noise, and the coded level the GPU test
(tests/test_mimo_gpu.py) runs at."""
import os
import re

import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import diversity_ref as DR
from tests import ldpc_ref as R
from tests import mimo_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTS, BITS = orc.qpsk_table()
LEVELS_DB = (14.0, 12.0, 10.0)                             # the three noise levels of the coded test, 2 dB apart
LEVEL_DB = 14.0                                            # what it settles: tests/test_mimo_gpu.py runs at this level


def test_interface_is_declared():
    """gf3_mimo_pilots, gf3_mimo_detect and GF3_MIMO_STREAMS: in the header, in the ctypes table, in the build's unit list."""
    from gf3_audio_modem_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gf3rx.h")).read()
    for name in ("gf3_mimo_pilots", "gf3_mimo_detect"):
        assert re.search(rf"\bint\s+{name}\s*\(", hdr)
        assert name in _lib.exported_names()
    m = re.search(r"#define\s+GF3_MIMO_STREAMS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 2 == _lib.GF3_MIMO_STREAMS
    assert "gf3rx_mimo" in build.UNITS and os.path.exists(os.path.join(build.CSRC, "gf3rx_mimo.hip"))


def test_facade_refuses_without_gpu():
    from gf3_audio_modem_amd.OFDM import receiver
    x = np.zeros(1000)

    def rx(**attrs):
        r = receiver("A2", encoding=attrs.pop("encoding", "QCLDPC-1/2"), no_pilots=attrs.pop("no_pilots", 20), packet_length=20)
        for k, v in attrs.items():
            setattr(r, k, v)
        return r
    for P in (0, 1, 3, 21):
        with pytest.raises(ValueError, match="no_pilots"):
            rx(no_pilots=P).receive_mimo([x, x])
        with pytest.raises(ValueError, match="no_pilots"):
            rx(no_pilots=P).transmit_mimo(np.zeros(100, dtype=np.int64))
    for signals in ([], [x], [x] * 5, np.zeros((1, 100)), np.zeros((5, 100))):
        with pytest.raises(ValueError, match="2 to 4 recordings"):
            rx().receive_mimo(signals)
    with pytest.raises(ValueError, match="2-D array"):
        rx().receive_mimo(x)
    for weighting in ("noise", "noise2d", "flat"):
        with pytest.raises(ValueError, match="llr_weighting"):
            rx(llr_weighting=weighting).receive_mimo([x, x])
    for name, value in (("fused_llr", True), ("phase_tracking", True), ("decoder_feedback", 1), ("interleave", True)):
        with pytest.raises(ValueError, match=name):
            rx(**{name: value}).receive_mimo([x, x])
    with pytest.raises(ValueError, match="bit_loading"):
        rx(bit_loading=np.full(1400, 2, dtype=np.uint8)).receive_mimo([x, x])
    for advance in (-1, 225, 1.5, True, None, "48"):
        with pytest.raises(ValueError, match="mimo_advance"):
            rx(mimo_advance=advance).receive_mimo([x, x])
    with pytest.raises(NotImplementedError, match="impulse_blanking"):
        rx(impulse_blanking=True).receive_mimo([x, x])
    with pytest.raises(NotImplementedError, match="channel_denoising"):
        rx(channel_denoising=True).receive_mimo([x, x])
    with pytest.raises(NotImplementedError, match="plots"):
        rx().receive_mimo([x, x], graph_output=True)
    with pytest.raises(NotImplementedError, match="piece-wise"):
        rx(host_chunk_samples=1 << 20).receive_mimo([x, x])
    # the transmit side
    with pytest.raises(ValueError, match="interleave"):
        rx(interleave=True).transmit_mimo(np.zeros(100, dtype=np.int64))
    with pytest.raises(NotImplementedError, match="bit_loading"):
        rx(bit_loading=np.full(1400, 2, dtype=np.uint8)).transmit_mimo(np.zeros(100, dtype=np.int64))
    with pytest.raises(NotImplementedError, match="papr_reduction"):
        rx(papr_reduction=True).transmit_mimo(np.zeros(100, dtype=np.int64))
    r = rx()
    assert r.mimo_advance == 48 and r.last_mimo_separation is None and r.last_branch_starts is None


def small_params(P=2, D=5):
    """N = 1024, CP = 64, data bins 5 .. 399 (C = 395), the reference's QPSK, seeded pilot bits"""
    known = np.random.default_rng(99).integers(0, 2, size=1024).astype(np.uint8)
    return orc.RxParams(N=1024, CP=64, P=P, D=D, lo=5, hi=400, const_points=PTS, const_bits=BITS, known_bits=known, fit_lo=10, fit_hi=300)


def small_scenario(P=2):
    """Two packets per speaker of seeded bits through the scenario's room -> (p, bits, the speakers' streams, recordings)"""
    p = small_params(P)
    bits = np.random.default_rng(3).integers(0, 2, size=4 * p.D * p.C * p.mu)
    tx2 = MR.tx_mimo(bits, np.full(p.K - p.C, (1 + 1j) / np.sqrt(2)), p, lead=300, tail=400)
    return p, bits, tx2, MR.through(tx2)


@pytest.mark.parametrize("P", [2, 4])
def test_cover_identity(P):
    """Cover 0 of the restated pilot estimate is oracle.ls_estimate on the same stream -- the plain mean over the pilot
    symbols, what the demodulator returns as Hs / He -- and it is speaker 0's channel alone: with speaker 1 switched off
    the same samples give the same column 0 to rounding, and column 1 vanishes."""
    p, bits, tx2, clean = small_scenario(P)
    r = clean[0]
    st = orc.frame_starts(orc.chirp_method(r, p)) - 16
    H, status = MR.pilots(r, st, p)
    assert not status.any() and H.shape == (2, 2, 2, p.K)
    X = orc.demod_fft(orc.gather_frames(r, st, p).astype(np.float64), p)
    _, start, end = orc.split_pilots(X, p)
    Hs, He = orc.ls_estimate(start, end, p)
    np.testing.assert_allclose(H[:, 0, 0], Hs, rtol=1e-12)
    np.testing.assert_allclose(H[:, 1, 0], He, rtol=1e-12)
    alone = MR.through(np.stack([tx2[0], np.zeros_like(tx2[1])]))[0]
    H0, _ = MR.pilots(alone, st, p)
    scale = np.abs(H0[:, :, 0]).max()
    assert np.abs(H0[:, :, 0] - H[:, :, 0]).max() < 1e-12 * scale and np.abs(H0[:, :, 1]).max() < 1e-12 * scale
    # a packet cut off at either end: status 1 and NaN rows, the neighbour untouched
    Hc, sc = MR.pilots(r, np.array([-1, st[0], len(r) - p.M * p.S + 1]), p)
    assert sc.tolist() == [1, 0, 1] and np.isnan(Hc[[0, 2]]).all() and np.array_equal(Hc[1], H[0])


def test_scenario_needs_the_advance():
    """Noiseless, both streams come back exact with the window moved back by 16 samples, and do NOT without the advance:
    speaker 1 arrives 6 samples ahead of the chirp's lock at microphone 0, so an unmoved window takes the last 6 samples of
    every symbol from the next one.  (Measured: 0 and 30 bit errors of 15800.)  In noise the joint detector beats zero
    forcing on the same statistics (measured, ML | ZF bit errors: 20 dB 3 | 246, 12 dB 52 | 844); median separation 0.30."""
    p, bits, tx2, clean = small_scenario()
    o = MR.receive_mimo(clean, p, advance=16)
    assert o["starts"].shape == (2, 2) and np.array_equal(o["bits"], bits)
    assert o["llr"].dtype == np.float32 and o["llr"].shape == bits.shape
    bare = MR.receive_mimo(clean, p, advance=0)
    print(f"bit errors without the advance: {int(np.sum(bare['bits'] != bits))} of {len(bits)}; "
          f"median separation {np.median(o['separation']):.2f}")
    assert not np.array_equal(bare["bits"], bits)
    # the signs are the joint argmin's labels wherever the LLR is not a tie
    lab = BITS[o["pair"]]                                   # [F, 2, D, C, mu]
    llr = o["llr"].reshape(lab.shape)
    assert np.array_equal((llr < 0)[llr != 0], lab.astype(bool)[llr != 0])
    for snr in (20.0, 12.0):
        n = MR.receive_mimo(MR.add_noise(clean, tx2, snr), p, advance=16)
        zf = MR.zero_forcing(n["Y"], n["H"], n["slopes"], p).reshape(-1) < 0
        ml_errors, zf_errors = int(np.sum(n["bits"] != bits)), int(np.sum(zf != bits))
        print(f"{snr} dB: ML {ml_errors}, zero forcing {zf_errors} bit errors of {len(bits)}")
        assert ml_errors < zf_errors


def coded_scenario():
    """The GPU test's geometry (mode A3, no_pilots 4, packet_length 4: N = 4096, CP = 224, C = 900): one packet pair of 9
    seeded rate-1/2 codewords and 576 seeded fill bits, constant filler, through the scenario's room
    -> (p, shift table, messages, coded bits, the speakers' streams, clean recordings)"""
    from gf3_audio_modem_amd.ldpc import shift_table
    from gf3_audio_modem_amd.OFDM import receiver
    known = np.asarray(receiver("A3").known_sequence, dtype=np.uint8)
    p = orc.RxParams(N=4096, CP=224, P=4, D=4, lo=100, hi=1000, const_points=PTS, const_bits=BITS, known_bits=known)
    sh = shift_table("1/2")
    k = (sh.shape[1] - sh.shape[0]) * 64
    rng = np.random.default_rng(7)
    msg = rng.integers(0, 2, size=(9, k), dtype=np.uint8)
    coded = np.concatenate([R.encode(sh, msg).reshape(-1), rng.integers(0, 2, size=2 * p.D * p.C * 2 - 9 * 1536, dtype=np.uint8)])
    tx2 = MR.tx_mimo(coded, np.full(p.K - p.C, (1 + 1j) / np.sqrt(2)), p, lead=300, tail=400)
    return p, sh, msg, coded, tx2, MR.through(tx2)


def test_coded_level():
    """"QCLDPC-1/2" over the scenario's room, the default advance of 48 samples, white noise (seeds 20, 21) below the RMS of
    a packet body as one speaker sends it; the restated chain with the restated decoder, 50 iterations.  Failed codewords
    of 9, raw bit error rate of the joint detector | of zero forcing on the same statistics:
        14 dB:   0    0.17 % | 4.2 %
        12 dB:   0    0.35 % | 5.2 %
        10 dB:   9    30.9 % | 37.7 %
    At 10 dB nothing is left: the reference's slope fit on microphone 1 slips a cycle at a null of its channel from speaker 0
    (slope -0.0188 instead of 1e-5), and with it the channel model of every data symbol; that fit is the demodulator's own
    and is not this feature's.  The highest noise that fails no codeword and whose next noisier level fails none either is
    14 dB: LEVEL_DB, which tests/test_mimo_gpu.py runs at."""
    p, sh, msg, coded, tx2, clean = coded_scenario()
    failed = []
    for snr in LEVELS_DB:
        o = MR.receive_mimo(MR.add_noise(clean, tx2, snr), p)
        assert o["starts"].shape == (2, 1)
        failed.append(DR.failed(sh, o["llr"], msg))
        print(f"{snr} dB: failed {failed[-1]} of 9, raw BER {np.mean(o['bits'] != coded):.4f}")
    assert failed[:2] == [0, 0]
    settled = [a for a, n, m in zip(LEVELS_DB, failed, failed[1:]) if n == 0 and m == 0]
    assert settled and settled[-1] == LEVEL_DB
