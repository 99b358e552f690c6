"""Receive windowing (every symbol tapered into its cyclic prefix ahead of the demodulator), host side (no GPU): the declared
interface, the façade's refusals, the properties of the NumPy restatement (tests/window_ref.py), and the interferer scenario
that settles the tone level the GPU test (tests/test_window_gpu.py) runs at."""
import dataclasses
import functools
import os
import re

import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import diversity_ref as DR
from tests import ldpc_ref as R
from tests import window_ref as WR
from tests.util import modeA2_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS_DB = (12.0, 14.0, 16.0, 18.0)                       # the tone levels of the scenario, 2 dB apart, ascending
LEVEL_DB = 16.0                                            # what it settles: tests/test_window_gpu.py runs at this level
PACKETS = 2


def test_interface_is_declared():
    """gf3_window_frames: in the header, in the ctypes table with its eleven arguments, in the build's unit list."""
    import ctypes as C
    from gf3_audio_modem_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gf3rx.h")).read()
    assert re.search(r"\bint\s+gf3_window_frames\s*\(", hdr)
    res, args = _lib._SIGS["gf3_window_frames"]
    assert res is C.c_int and len(args) == 11 and args[2] is C.c_int64 and args[4] is C.c_int64 and args[6] is C.c_int32
    assert "gf3_window_frames" in _lib.exported_names()
    unit = os.path.join(build.CSRC, "gf3rx_window.hip")
    assert "gf3rx_window" in build.UNITS and unit in build.SRC and "gf3_window_frames" in open(unit).read()


def test_facade_refuses_without_gpu():
    from gf3_audio_modem_amd import Engine
    from gf3_audio_modem_amd.OFDM import receiver
    x = np.zeros(1000)

    def rx(**attrs):
        r = receiver("A2", encoding=attrs.pop("encoding", "QCLDPC-1/2"), no_pilots=4, packet_length=8)
        for k, v in attrs.items():
            setattr(r, k, v)
        return r
    r = rx()
    assert r.receive_window == 0 and r.last_window_report is None and r.cp_length == 224
    calls = (lambda r: r.receive(x), lambda r: r.receive_diversity([x, x]), lambda r: r.receive_mimo([x, x]),
             lambda r: r.receive_stbc([x]))
    for bad in (-1, 225, 1.5, True, None, "64"):
        with pytest.raises(ValueError, match="receive_window"):
            Engine.check_window(bad, 224)
        for call in calls:
            with pytest.raises(ValueError, match="receive_window must be an integer"):
                call(rx(receive_window=bad))
    assert Engine.check_window(0, 224) == 0 and Engine.check_window(np.int64(224), 224) == 224
    # the advance and the window are spent from the same prefix
    for call in calls[2:]:
        with pytest.raises(ValueError, match=r"mimo_advance \+ receive_window = 48 \+ 177 samples exceed cp_length = 224"):
            call(rx(receive_window=177))
        with pytest.raises(ValueError, match="mimo_advance"):
            call(rx(receive_window=224, mimo_advance=1))
    # the piece-wise host path
    with pytest.raises(NotImplementedError, match="receive_window: .*piece-wise host path.* has no windowing pass; receive shorter recordings"):
        rx(encoding="None", receive_window=64, host_chunk_samples=1 << 20).receive(x)
    with pytest.raises(NotImplementedError, match="receive_diversity: .*combines nothing"):
        rx(receive_window=64, host_chunk_samples=1 << 20).receive_diversity([x, x])
    # the plan carries the taper, last and with its default
    from gf3_audio_modem_amd.pipeline import ReceivePlan, plan_receive, plan_stbc
    assert ReceivePlan._fields[-1] == "window" and ReceivePlan._field_defaults["window"] == 0
    r = rx(receive_window=64)
    assert plan_receive(r, r._chain(), [1000], False, False).window == 64
    assert plan_receive(r, r._chain(), [1000, 1000], False, True).window == 64
    assert plan_stbc(r, r._chain(), [1000], False).window == 64
    assert plan_receive(rx(), rx()._chain(), [1000], False, False).window == 0


@pytest.mark.parametrize("L", [1, 2, 3, 55, 56, 128])
def test_ramp_is_nyquist(L):
    from gf3_audio_modem_amd import Engine
    r = WR.ramp(L)
    assert np.array_equal(r, Engine.window_ramp(L)) and r.shape == (L,) and (r > 0).all() and (r < 1).all()
    assert np.abs(r + r[::-1] - 1.0).max() <= 2.0 ** -52
    assert (np.diff(r) > 0).all()


@pytest.mark.parametrize("N, CP, L", [(1024, 56, 1), (1024, 56, 55), (1024, 56, 56), (4096, 224, 128), (4096, 1184, 1184)])
def test_a_periodic_signal_passes_unchanged(N, CP, L):
    """A symbol that is periodic in N over [CP - L, S) -- what a channel shorter than CP - L leaves of a transmitted symbol --
    comes back as it was: out = a (1 - r) + a r, three roundings of which none exceeds 2^-53 |a|, and the report's mismatch
    is exactly 0.  The samples ahead of CP - L need not be periodic (the channel's transient lives there)."""
    rng = np.random.default_rng(N + L)
    S = N + CP
    sym = rng.normal(0.0, 3.0, size=(3, S))
    sym[:, CP - L: CP] = sym[:, S - L:]
    out, rep = WR.window_symbols(sym, N, CP, L)
    err = np.abs(out - sym)
    print(f"N {N} CP {CP} L {L}: largest change {err.max():.3e}")
    assert (err <= 3 * 2.0 ** -53 * np.abs(sym)).all()
    assert np.array_equal(out[:, : S - L], sym[:, : S - L])
    assert (rep[:, 0] == 0.0).all() and np.allclose(rep[:, 1], 2 * (sym[:, S - L:] ** 2).sum(axis=1), rtol=1e-14)
    # and what is not periodic is seen through the window: a symbol of ones in front of a symbol of zeros
    edge = np.zeros((1, S))
    edge[0, :CP] = 1.0
    out, rep = WR.window_symbols(edge, N, CP, L)
    assert np.array_equal(out[0, S - L:], WR.ramp(L)) and rep[0, 0] == L and rep[0, 1] == L


def test_restatement_rows_statuses_and_nonfinite():
    N, CP, M, L = 64, 8, 3, 5
    S = N + CP
    rng = np.random.default_rng(1)
    x = rng.normal(size=4 * M * S)
    x[10 + S + S - 2] = np.nan                               # packet at 10: symbol 1's ramp
    x[10 + 2 * S + CP - 1] = np.inf                          # symbol 2's folded stretch
    x[10 + 1] = np.inf                                       # symbol 0, outside both stretches: copied, not in the report
    starts = [10, -1, len(x) - M * S, len(x) - M * S + 1]
    rows, raw, status, report = WR.window_rows(x, starts, N, CP, M, L)
    assert status.tolist() == [0, 1, 0, 1] and rows.shape == (4, M * S)
    assert not rows[1].any() and not rows[3].any() and np.isnan(report[1]).all() and np.isnan(report[3]).all()
    assert np.isfinite(report[0, 0]).all() and np.isnan(report[0, 1:]).all() and np.isfinite(report[2]).all()
    bad = ~np.isfinite(rows[0])
    assert np.flatnonzero(bad).tolist() == [1, S + S - 2, 2 * S + CP - 1, 2 * S + S - 1]
    d = WR.mismatch_db(report)
    assert np.isnan(d[[0, 1, 3]]).all() and -1.0 < d[2] < 4.0                 # (independent stretches: 10 log10(2 / 2) = 0 dB)
    for dtype, lo, hi in ((np.int16, -30000, 30001), (np.uint8, 0, 256)):
        xi = rng.integers(lo, hi, size=2 * M * S).astype(dtype)
        rows, raw, _, report = WR.window_rows(xi, [7], N, CP, M, L)
        assert rows.dtype == dtype and np.abs(rows.astype(np.float64) - raw).max() <= 0.5
        assert np.array_equal(report, np.rint(report))


@functools.lru_cache(maxsize=None)
def scenario():
    """Mode A2 with no_pilots = 4 and packet_length = 8 (N = 4096, CP = 224, C = 1400): PACKETS packets of seeded rate-1/2
    codewords (29 in two packets) and seeded fill bits, constant filler, through window_ref.channel()
    -> (p, shift table, messages, coded bits, the points sent [F D, C], the clean recording, its RMS over the bodies)"""
    from gf3_audio_modem_amd.ldpc import shift_table
    from gf3_audio_modem_amd.OFDM import receiver
    known = np.asarray(receiver("A2").known_sequence, dtype=np.uint8)
    p = dataclasses.replace(modeA2_params(known), P=4, D=8)
    sh = shift_table("1/2")
    k = (sh.shape[1] - sh.shape[0]) * 64
    per = p.D * p.C * p.mu
    n_cw = PACKETS * per // 1536
    rng = np.random.default_rng(11)
    msg = rng.integers(0, 2, size=(n_cw, k), dtype=np.uint8)
    coded = np.concatenate([R.encode(sh, msg).reshape(-1), rng.integers(0, 2, size=PACKETS * per - n_cw * 1536, dtype=np.uint8)])
    tx = orc.tx_stream(coded, np.full(p.K - p.C, (1 + 1j) / np.sqrt(2)), p, lead=WR.LEAD, tail=WR.TAIL)
    clean = np.convolve(tx, WR.channel())[: len(tx)]
    sent = orc.map_bits(coded.reshape(-1, p.C, p.mu), p)
    return p, sh, msg, coded, sent, clean, WR.body_rms(clean, p, PACKETS)


def test_interferer_level():
    """Why the feature.  "QCLDPC-1/2" with the noise weights over a channel of 40 taps, white noise 25 dB below the recording's
    body RMS, one tone at 9005.3 Hz -- off the carrier grid -- whose power lies `level` dB above the body's; the restated
    chain with the restated decoder, 50 iterations, without the window and with L = 128.  The figures are printed: failed
    codewords, the median per-carrier SINR and the carriers below 10 dB.  Measured, failed codewords of 29 (median SINR,
    carriers of 1400 below 10 dB):

        tone      rectangular              L = 128
        12 dB      5  (9.1 dB,  750)       0  (19.2 dB, 162)
        14 dB     13  (7.4 dB,  859)       0  (19.1 dB, 163)
        16 dB     15  (5.5 dB, 1025)       0  (19.1 dB, 167)
        18 dB     17  (3.6 dB, 1175)      14  (-0.3 dB, 1400: one packet lost whole)

    The report's mismatch is +2.5 .. +2.8 dB at every level:
    the tone itself is what does not repeat after N samples, and it outweighs the signal.
    LEVEL_DB is the lowest level at which the rectangular window loses at least half its codewords while L = 128 decodes
    all: 16 dB, which tests/test_window_gpu.py runs at.  What ends the window's reach at 18 dB is not leakage: the tone lies
    at carrier 768, inside the range 500 .. 1000 over which the reference fits the phase slope between the pilot blocks
    on separately unwrapped angles, and once the tone owns a few carriers of an estimate the unwrapping slips a cycle there
    (slope -0.0188 instead of 1e-5) and takes the packet's channel model with it.  That fit is the demodulator's own and
    fails under the rectangle too (from 20 dB on in this scenario, at lower levels with other channels)."""
    p, sh, msg, coded, sent, clean, rms = scenario()
    n_cw = len(msg)
    plain, windowed = [], []
    for level in LEVELS_DB:
        r = WR.interfered(clean, rms, level)
        for L, into in ((0, plain), (WR.TAPER, windowed)):
            o = WR.receive(r, p, L)
            assert o["starts"].shape == (PACKETS,)
            into.append(DR.failed(sh, DR.single_llrs(o, "noise", p), msg))
            s = WR.sinr_db(o["eq"], sent)
            print(f"tone {level:+.0f} dB, L = {L}: failed {into[-1]} of {n_cw}, median SINR {np.median(s):.1f} dB, "
                  f"{int((s < 10.0).sum())} of {p.C} carriers below 10 dB"
                  + (f", mismatch {WR.mismatch_db(o['report']).round(1).tolist()} dB" if L else ""))
    settled = [lv for lv, a, b in zip(LEVELS_DB, plain, windowed) if 2 * a >= n_cw and b == 0]
    assert settled and settled[0] == LEVEL_DB
