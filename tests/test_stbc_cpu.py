"""Transmit diversity (two speakers, one microphone, the Alamouti code over pairs of data symbols), host side (no GPU): the
declared interface, the façade's refusals, the time-reversal identity the wire format rests on, the NumPy restatement
(tests/stbc_ref.py) noiseless and in noise against one speaker and against the mono signal on both speakers, over the rooms
of tests/mimo_ref.py, and the coded level the GPU test (tests/test_stbc_gpu.py) runs at."""
import os
import re

import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import diversity_ref as DR
from tests import mimo_ref as MR
from tests import stbc_ref as SR
from tests.test_mimo_cpu import coded_scenario, small_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = (1 + 1j) / np.sqrt(2)
LEVELS_DB = (10.0, 8.0, 6.0, 4.0)                           # the noise levels of the coded test, 2 dB apart
LEVEL_DB = 8.0                                             # what it settles: tests/test_stbc_gpu.py runs at this level
ROOM, MIC = None, 1                                        # the coded test's room (mimo_ref.channel()) and its one microphone


def test_interface_is_declared():
    """gf3_stbc_slope and gf3_stbc_detect: in the header, in the ctypes table, in the build's unit list."""
    from gf3_audio_modem_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gf3rx.h")).read()
    for name in ("gf3_stbc_slope", "gf3_stbc_detect"):
        assert re.search(rf"\bint\s+{name}\s*\(", hdr)
        assert name in _lib.exported_names()
    assert "gf3rx_stbc" in build.UNITS and os.path.exists(os.path.join(build.CSRC, "gf3rx_stbc.hip"))


def test_facade_refuses_without_gpu():
    from gf3_audio_modem_amd.OFDM import receiver
    x = np.zeros(1000)
    bits = np.zeros(100, dtype=np.int64)

    def rx(**attrs):
        r = receiver("A2", encoding=attrs.pop("encoding", "QCLDPC-1/2"), no_pilots=attrs.pop("no_pilots", 20),
                     packet_length=attrs.pop("packet_length", 20))
        for k, v in attrs.items():
            setattr(r, k, v)
        return r
    for P in (0, 1, 3, 21):
        with pytest.raises(ValueError, match="no_pilots"):
            rx(no_pilots=P).receive_stbc([x])
        with pytest.raises(ValueError, match="no_pilots"):
            rx(no_pilots=P).transmit_stbc(bits)
    for D in (1, 19):
        with pytest.raises(ValueError, match="packet_length must be even"):
            rx(packet_length=D).receive_stbc([x])
        with pytest.raises(ValueError, match="packet_length must be even"):
            rx(packet_length=D).transmit_stbc(bits)
    for signals in ([], [x] * 5, np.zeros((0, 100)), np.zeros((5, 100))):
        with pytest.raises(ValueError, match="1 to 4 recordings"):
            rx().receive_stbc(signals)
    with pytest.raises(ValueError, match="2-D array"):
        rx().receive_stbc(x)
    for weighting in ("noise", "noise2d", "flat"):
        with pytest.raises(ValueError, match="receive_stbc: llr_weighting"):
            rx(llr_weighting=weighting).receive_stbc([x])
    for name, value in (("fused_llr", True), ("phase_tracking", True), ("decoder_feedback", 1), ("interleave", True)):
        with pytest.raises(ValueError, match=f"receive_stbc: {name}"):
            rx(**{name: value}).receive_stbc([x])
    with pytest.raises(ValueError, match="receive_stbc: bit_loading"):
        rx(bit_loading=np.full(1400, 2, dtype=np.uint8)).receive_stbc([x])
    for advance in (-1, 225, 1.5, True, None, "48"):
        with pytest.raises(ValueError, match="mimo_advance"):
            rx(mimo_advance=advance).receive_stbc([x])
    with pytest.raises(NotImplementedError, match="receive_stbc: impulse_blanking"):
        rx(impulse_blanking=True).receive_stbc([x])
    with pytest.raises(NotImplementedError, match="receive_stbc: channel_denoising"):
        rx(channel_denoising=True).receive_stbc([x])
    with pytest.raises(NotImplementedError, match="receive_stbc: no plots"):
        rx().receive_stbc([x], graph_output=True)
    with pytest.raises(NotImplementedError, match="receive_stbc: .*piece-wise"):
        rx(host_chunk_samples=1 << 20).receive_stbc([x])
    # the transmit side
    with pytest.raises(ValueError, match="transmit_stbc: interleave"):
        rx(interleave=True).transmit_stbc(bits)
    with pytest.raises(NotImplementedError, match="transmit_stbc with bit_loading"):
        rx(bit_loading=np.full(1400, 2, dtype=np.uint8)).transmit_stbc(bits)
    with pytest.raises(NotImplementedError, match="transmit_stbc with papr_reduction"):
        rx(papr_reduction=True).transmit_stbc(bits)
    r = rx()
    assert r.last_stbc_slope is None and r.last_branch_starts is None
    # receive_mimo's own refusals read as they did
    with pytest.raises(ValueError, match="receive_mimo: interleave is not supported with two streams; switch it off"):
        rx(interleave=True).receive_mimo([x, x])
    with pytest.raises(NotImplementedError, match="receive_mimo: .* separates nothing; receive shorter recordings"):
        rx(host_chunk_samples=1 << 20).receive_mimo([x, x])


def test_time_reversal_is_the_conjugate_spectrum():
    """A real symbol reversed in time, x[(-n) mod N], has the conjugate spectrum; with its prefix rebuilt it is what the
    oracle's transmitter makes of the conjugate points.  In tx_stbc's streams, slot 2j + 1 of speaker 0 therefore carries
    -conj(X_(2j+1)) and that of speaker 1 conj(X_2j), slot 2j the plain X_2j and X_(2j+1)."""
    p = small_params(P=2, D=6)
    rng = np.random.default_rng(5)
    x = rng.normal(size=(3, p.S))
    x[:, :p.CP] = x[:, p.N:]                                # a symbol under its prefix
    rev = SR.reversed_symbols(x, p)
    assert np.array_equal(rev[:, :p.CP], rev[:, p.N:])
    X, R = np.fft.rfft(x[:, p.CP:]), np.fft.rfft(rev[:, p.CP:])
    assert np.abs(R - np.conj(X)).max() <= 1e-12 * np.abs(X).max()
    bits = rng.integers(0, 2, size=p.D * p.C * p.mu)
    fill = rng.choice(np.array([1, -1, 1j, -1j]) * FILL, size=p.K - p.C)
    tx2 = SR.tx_stbc(bits, fill, p)
    plain = orc.tx_frames(bits, fill, p)[0, p.Lc:].reshape(p.M, p.S)[p.P: p.P + p.D, p.CP:]
    Xl = np.fft.fft(plain)
    got = [np.fft.fft(t[p.Lc: p.Lc + p.M * p.S].reshape(p.M, p.S)[p.P: p.P + p.D, p.CP:]) for t in tx2]
    tol = 1e-12 * np.abs(Xl).max()
    assert np.abs(got[0][0::2] - Xl[0::2]).max() <= tol and np.abs(got[1][0::2] - Xl[1::2]).max() <= tol
    assert np.abs(got[0][1::2] + np.conj(Xl[1::2])).max() <= tol and np.abs(got[1][1::2] - np.conj(Xl[0::2])).max() <= tol
    # chirps, pilots and cover are tx_mimo's
    assert not tx2[1, :p.Lc].any() and not tx2[1, p.Lc + p.M * p.S:].any()
    body = [t[p.Lc: p.Lc + p.M * p.S].reshape(p.M, p.S) for t in tx2]
    sign = MR.cover(p.P)[1][:, None]
    assert np.array_equal(body[1][:p.P], body[0][:p.P] * sign) and np.array_equal(body[1][p.P + p.D:], body[0][p.P + p.D:] * sign)


def small_case(P=2, D=6):
    """`small_params` with D = 6 and 4 packets of seeded bits (18 960 with P = 2) -> (p, bits, constant filler)"""
    p = small_params(P, D)
    bits = np.random.default_rng(3).integers(0, 2, size=4 * p.D * p.C * p.mu)
    return p, bits, np.full(p.K - p.C, FILL)


@pytest.mark.parametrize("P", [2, 4])
def test_noiseless_is_exact(P):
    """Through the static room, window advance 16: each microphone alone and both together return every bit, and the cross
    term G01 -- what a change of the channel between the two slots of a pair would leave -- is rounding (measured: 1e-16
    to 2.5e-16 of the mean G00; the bound is 1e-12)."""
    p, bits, fill = small_case(P)
    clean = MR.through(SR.tx_stbc(bits, fill, p, lead=300, tail=400))
    for mics in ([0], [1], [0, 1]):
        o = SR.receive_stbc([clean[b] for b in mics], p, advance=16)
        assert o["starts"].shape == (len(mics), 4) and o["llr"].dtype == np.float32
        assert np.array_equal(o["bits"], bits), mics
        G00, _, G01 = o["stats"][:3]
        print(f"P {P}, microphones {mics}: max |G01| / mean G00 = {np.abs(G01).max() / G00.mean():.2e}, slope {o['slope'][0]:.2e}")
        assert np.abs(G01).max() <= 1e-12 * G00.mean()
        lab = np.asarray(p.const_bits)[o["pair"]]           # the signs are the joint argmin's labels wherever the LLR is no tie
        llr = o["llr"].reshape(lab.shape)
        assert np.array_equal((llr < 0)[llr != 0], lab.astype(bool)[llr != 0])


def test_one_microphone_in_noise_against_the_alternatives():
    """Why the feature.  `small_params`, D = 6, 4 packets, 18 960 bits, window advance 16; rooms mimo_ref.channel(seed),
    seeds 1 .. 8, each microphone alone: 16 cases; white noise (seed 20 + microphone) 14 dB below one speaker's body RMS.
    Hard-decision errors summed over the 16 cases, measured:

        scheme                                             14 dB      10 dB
        Alamouti, joint slope                                366      5 839
        one speaker (the oracle's receive)                11 006     23 027
        the mono signal on both speakers                   7 142     16 627
        Alamouti with the reference's single-path slope    8 782     18 783

    The worst single Alamouti case at 14 dB is 175 errors (0.92 % of the bits).  The last row is the same detector on the
    same samples with the slope the reference fits on ONE path (speaker 0's): that fit slips a cycle at that path's nulls
    and loses whole packets, which is why the slope is fitted on the product summed over both paths.  (At 10 dB one case,
    room 4 at microphone 0, holds 4 644 of the Alamouti row's errors: there the joint fit slips too.)
    Asserted at 14 dB: the Alamouti total is below half of each of the other three; no case exceeds 2 % of the bits."""
    p, bits, fill = small_case()
    txs = {"alamouti": SR.tx_stbc(bits, fill, p, lead=300, tail=400), "one": SR.single_speaker(bits, fill, p, lead=300, tail=400),
           "mono": SR.mono(bits, fill, p, lead=300, tail=400)}
    rms = SR.body_rms(txs["alamouti"])
    total = dict(alamouti=0, one=0, mono=0, reference_slope=0)
    worst = 0
    for seed in range(1, 9):
        h = MR.channel(seed)
        heard = {k: MR.through(v, h) for k, v in txs.items()}
        for mic in (0, 1):
            noisy = SR.add_noise([heard["alamouti"][mic]], rms, 14.0, [mic])
            e = int(np.sum(SR.receive_stbc(noisy, p, advance=16)["bits"] != bits))
            total["alamouti"] += e
            worst = max(worst, e)
            total["reference_slope"] += int(np.sum(SR.receive_stbc(noisy, p, advance=16, slope="reference")["bits"] != bits))
            for k in ("one", "mono"):
                noisy = SR.add_noise([heard[k][mic]], rms, 14.0, [mic])
                total[k] += int(np.sum(SR.receive_single(noisy[0], p, 16)["bits"] != bits))
    print(f"14 dB, errors of 16 x {len(bits)} bits: {total}; worst Alamouti case {worst}")
    for k in ("one", "mono", "reference_slope"):
        assert 2 * total["alamouti"] < total[k], k
    assert worst <= 0.02 * len(bits)


def stbc_coded_scenario():
    """tests/test_mimo_cpu.py's coded geometry (mode A3, no_pilots 4, packet_length 4: N = 4096, CP = 224, C = 900) and its
    bits -- two packets of 9 seeded rate-1/2 codewords and 576 fill bits -- as ONE stream -> (p, shift table, messages,
    coded bits, the Alamouti streams, the one-speaker streams, one speaker's body RMS)"""
    p, sh, msg, coded, _, _ = coded_scenario()
    fill = np.full(p.K - p.C, FILL)
    tx2 = SR.tx_stbc(coded, fill, p, lead=300, tail=400)
    return p, sh, msg, coded, tx2, SR.single_speaker(coded, fill, p, lead=300, tail=400), SR.body_rms(tx2)


def test_coded_level():
    """"QCLDPC-1/2" over the room mimo_ref.channel(), microphone 1 ALONE, the default advance of 48 samples, white noise
    (seed 21) below one speaker's body RMS; the restated chains with the restated decoder, 50 iterations.  Failed codewords
    of 9 (raw bit error rate), measured:

        level    Alamouti, joint slope    one speaker, CSI-weighted max-log LLRs
        10 dB    0   (0.08 %)             5   (29.5 %)
         8 dB    0   (0.35 %)             5   (30.6 %)
         6 dB    0   (1.1 %)              0   (9.1 %)
         4 dB    0   (2.6 %)              9   (55.6 %)

    One speaker lives or dies on the reference's slope fit at the nulls of its one path (slope -0.0188 instead of 1e-5 at
    10 and 8 dB, right at 6 dB, +0.0188 at 4 dB).  (With mimo_ref.channel(7), microphone 0, one speaker fails 5 of 9 at
    12 dB and all 9 from 10 dB down; Alamouti fails none down to 4 dB.)  LEVEL_DB is the noisiest level at which Alamouti
    fails none, the next noisier level fails none either and one speaker fails at least one codeword: 8 dB, which
    tests/test_stbc_gpu.py runs at."""
    p, sh, msg, coded, tx2, one2, rms = stbc_coded_scenario()
    h = MR.channel() if ROOM is None else MR.channel(ROOM)
    heard, heard_one = MR.through(tx2, h)[MIC], MR.through(one2, h)[MIC]
    alamouti, one = [], []
    for snr in LEVELS_DB:
        o = SR.receive_stbc(SR.add_noise([heard], rms, snr, [MIC]), p)
        assert o["starts"].shape == (1, 2)
        s = SR.receive_single(SR.add_noise([heard_one], rms, snr, [MIC])[0], p, 48)
        alamouti.append(DR.failed(sh, o["llr"], msg))
        one.append(DR.failed(sh, DR.single_llrs(s, "csi", p), msg))
        print(f"{snr} dB: failed of 9: Alamouti {alamouti[-1]} (raw BER {np.mean(o['bits'] != coded):.4f}), "
              f"one speaker {one[-1]} (raw BER {np.mean(s['bits'] != coded):.4f}, slopes {s['slope']})")
    settled = [a for a, n, m, o1 in zip(LEVELS_DB, alamouti, alamouti[1:], one) if n == 0 and m == 0 and o1 >= 1]
    assert settled and settled[-1] == LEVEL_DB
