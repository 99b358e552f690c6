"""Whole-stream rate conversion, on the NumPy restatement (tests/rate_ref.py) and the host side of the package: what the
rule does to tones, the size of its coefficients, r = 1, block-wise against whole, the output counts of
Engine.stream_outputs against brute force, the ABI's names and the façade's refusals, which are raised before any GPU work.

Tone figures.  A unit tone at a fraction `frac` of the NARROWER of the two Nyquist frequencies is converted and compared
with the analytic tone at the outputs' times j r; the largest error over the outputs whose taps lie inside the input must
stay under -100 dB (1e-5) for frac up to 0.74 at T = 16 and 0.85 at T = 32.  At r = 2 and 4 a tone at (2 - 0.74 | 0.85) of the
output's Nyquist frequency, which would alias onto the edge of that band, must come out more than 105 dB down."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import rate_ref as QR

EDGE = {16: 0.74, 32: 0.85}
N_TONE = 3000


def tone_in(cycles_per_input_sample, phase=0.3):
    return np.cos(2.0 * np.pi * cycles_per_input_sample * np.arange(N_TONE) + phase)


def inner(r, T, n_out):
    """The outputs whose taps all lie inside N_TONE input samples."""
    j = np.arange(n_out)
    i = np.floor(j * r)
    Tw = QR.reach(r, T)
    return (i - Tw + 1 >= 0) & (i + Tw <= N_TONE - 1)


@pytest.mark.parametrize("T", [16, 32])
@pytest.mark.parametrize("r", QR.RATIOS, ids=lambda r: f"{r:.6g}")
def test_tones_in_the_passband_come_out_within_100_db(r, T):
    worst = 0.0
    for frac in (0.05, 0.4, 0.6, EDGE[T]):
        f_in = 0.5 * frac * (1.0 if r <= 1.0 else 1.0 / r)          # cycles per input sample
        raw, _ = QR.convert(tone_in(f_in), r, T)
        want = np.cos(2.0 * np.pi * f_in * (np.arange(len(raw)) * r) + 0.3)
        ok = inner(r, T, len(raw))
        assert ok.sum() > 200
        worst = max(worst, float(np.abs(raw - want)[ok].max()))
    print(f"r {r:.6g} T {T}: largest error {20 * np.log10(worst):.1f} dB")
    assert worst <= 1e-5


@pytest.mark.parametrize("T", [16, 32])
@pytest.mark.parametrize("r", [2.0, 4.0])
def test_tones_that_would_alias_are_rejected_by_105_db(r, T):
    f_in = 0.5 * (2.0 - EDGE[T]) / r
    raw, _ = QR.convert(tone_in(f_in), r, T)
    ok = inner(r, T, len(raw))
    worst = float(np.abs(raw)[ok].max())
    print(f"r {r} T {T}: a tone at {2.0 - EDGE[T]:.2f} of the output's Nyquist frequency comes out at {20 * np.log10(worst):.1f} dB")
    assert worst < 10.0 ** (-105.0 / 20.0)


def test_coefficient_sums_stay_below_four():
    for T in (16, 32):
        for r in QR.RATIOS + [1.0]:
            _, _, c = QR.coefficients(np.arange(4000, dtype=np.int64), r, T)
            s = float(np.abs(c).sum(axis=1).max())
            assert s < 4.0, (r, T, s)
            assert abs(float(c.sum(axis=1).mean()) - 1.0) < 1e-3, (r, T)        # unit gain at DC


def test_a_ratio_of_one_copies():
    x = np.random.default_rng(1).normal(0.0, 3.0, 700)
    for T in (16, 32):
        raw, _ = QR.convert(x, 1.0, T)
        assert np.array_equal(raw, x)
        raw, _ = QR.convert(x[100:300], 1.0, T, in_origin=100, j0=90, n_out=230)
        assert np.array_equal(raw, np.concatenate([np.zeros(10), x[100:300], np.zeros(20)]))


@pytest.mark.parametrize("r", [147 / 160, 160 / 147, 4.0, 44100.7 / 48000], ids=lambda r: f"{r:.6g}")
def test_blocks_give_the_bits_of_the_whole(r):
    x = np.random.default_rng(2).normal(0.0, 1.0, 2100)
    T = 16
    whole, _ = QR.convert(x, r, T)
    assert len(whole) == QR.whole_count(len(x), r)
    for sizes in ([1], [63], [64], [1000], [5, 700, 1, 1, 333, 64, 2, 900]):
        got = QR.convert_blocks(x, r, T, sizes)
        assert got.shape == whole.shape and np.array_equal(got.view(np.uint64), whole.view(np.uint64)), (r, sizes)


def test_single_sample_blocks_give_the_bits_of_the_whole_at_64_taps():
    x = np.random.default_rng(3).normal(0.0, 1.0, 400)
    for r, T in ((147 / 160, 32), (2.0, 32)):
        whole, _ = QR.convert(x, r, T)
        assert np.array_equal(QR.convert_blocks(x, r, T, [1]).view(np.uint64), whole.view(np.uint64))


def test_stream_outputs_against_brute_force():
    from gf3_audio_modem_amd.engine import Engine
    for T in (16, 32):
        for r in QR.RATIOS + [1.0, 0.3333333333333333, 3.999999999]:
            for n in list(range(0, 140)) + [511, 512, 513, 1500, 4095, 4096, 100003]:
                assert Engine.stream_outputs(n, r, T) == QR.final_count(n, r, T), (n, r, T)
                assert Engine.stream_outputs(n, r, T, final=True) == QR.whole_count(n, r), (n, r, T)
    # monotonic, and never beyond what a whole recording gives
    for r in (147 / 160, 160 / 147):
        a = [Engine.stream_outputs(n, r, 32) for n in range(300)]
        assert all(x <= y for x, y in zip(a, a[1:]))
        assert all(Engine.stream_outputs(n, r, 32) <= Engine.stream_outputs(n, r, 32, final=True) for n in range(300))
    assert Engine.stream_outputs(3 * 10 ** 12, 0.25, 16, final=True) == 4 * (3 * 10 ** 12 - 1) + 1
    for bad in (0.2, 4.5, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError, match="r must be"):
            Engine.stream_outputs(100, bad, 16)
    with pytest.raises(ValueError, match="half_taps"):
        Engine.stream_outputs(100, 1.0, 8)
    with pytest.raises(ValueError, match="n_seen"):
        Engine.stream_outputs(-1, 1.0, 16)


def test_abi_names_the_call():
    from gf3_audio_modem_amd import _lib, build
    assert "gf3_resample_stream" in _lib.exported_names()
    res, args = _lib._SIGS["gf3_resample_stream"]
    assert res is C.c_int and len(args) == 11 and args[5] is C.c_double and args[2] is C.c_int32
    hdr = open(os.path.join(os.path.dirname(build.CSRC), "..", "include", "gf3rx.h")).read()
    assert "int gf3_resample_stream(gf3_ctx *ctx, const void *d_in, int32_t in_dtype, int64_t n_in, int64_t in_origin, double r," in hdr
    assert any("gf3_resample_stream" in open(src).read() for src in build.SRC)


# ---- the façade's refusals: before any GPU work ---------------------------------------------------------------------
def rx_of(mode="A2", **attrs):
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver(mode, no_pilots=2, packet_length=4)
    for k, v in attrs.items():
        setattr(rx, k, v)
    return rx


def test_facade_defaults():
    rx = rx_of()
    assert rx.input_rate is None and rx.output_rate is None and rx.rate_taps == 64 and rx.last_input_rate is None
    plan = rx._plan([1000], False, False)
    assert plan.rates is None
    rx.input_rate = 48000                                           # fs itself: the same as None
    assert rx._plan([1000], False, False).rates is None
    rx.input_rate = [48000.0, 48000]
    assert rx._plan([1000, 1000], False, True).rates is None
    rx.input_rate, rx.rate_taps = 44100, 32
    assert rx_of("A3", input_rate=32000)._plan([10], False, False).rates == ((32000.0, 32),)
    assert rx._plan([1000], False, False).rates == ((44100.0, 16),)
    assert rx._plan([1000, 10], False, True).rates == ((44100.0, 16), (44100.0, 16))
    rx.input_rate = np.array([44100.0, 48000.0, 96000.0])
    assert rx._plan([5, 6, 7], False, True).rates == ((44100.0, 16), None, (96000.0, 16))


@pytest.mark.parametrize("bad", ["44100", 23999.9, 192000.5, float("nan"), float("inf"), -44100, True, [44100], (44100, 48000), 0])
def test_facade_refuses_a_bad_input_rate(bad):
    rx = rx_of(input_rate=bad)
    with pytest.raises(ValueError, match="input_rate"):
        rx.receive(np.zeros(5000))


def test_facade_refuses_bad_taps_rates_per_recording_and_a_band_that_does_not_fit():
    for taps in (16, 48, "64", True, None):
        with pytest.raises(ValueError, match="rate_taps"):
            rx_of(input_rate=44100, rate_taps=taps).receive(np.zeros(5000))
    with pytest.raises(ValueError, match="2 rates for 3 recordings"):
        rx_of(input_rate=[44100, 96000]).receive_diversity([np.zeros(5000)] * 3)
    with pytest.raises(ValueError, match="input_rate"):
        rx_of(input_rate=[44100, "x"]).receive_diversity([np.zeros(5000)] * 2)
    # A2's top data carrier, 1499 x 48000 / 4096 = 17 566 Hz, against half of 32 kHz (and of 35 132 Hz: exactly on it)
    for rate in (32000, 2 * 1499 * 48000 / 4096):
        with pytest.raises(ValueError, match="top data carrier"):
            rx_of(input_rate=rate).receive(np.zeros(5000))
    with pytest.raises(ValueError, match="top data carrier"):
        rx_of(input_rate=[44100, 32000]).receive_diversity([np.zeros(5000)] * 2)
    with pytest.raises(NotImplementedError, match="input_rate.*piece-wise host path"):
        rx_of(input_rate=44100, host_chunk_samples=1 << 22).receive(np.zeros(5000))
    # the value checks come first, as for the other options
    with pytest.raises(ValueError, match="input_rate"):
        rx_of(input_rate=1.0, host_chunk_samples=1 << 22).receive(np.zeros(5000))


def test_a_good_input_rate_passes_the_plan_and_reaches_the_engine():
    class Reached(Exception):
        pass

    def reached(*a, **kw):
        raise Reached
    for attrs in (dict(input_rate=44100), dict(input_rate=96000.0, rate_taps=32), dict(input_rate=np.float32(88200))):
        rx = rx_of(**attrs)
        rx._engine = reached
        with pytest.raises(Reached):
            rx.receive(np.zeros(5000, dtype=np.int16))


def test_transmitter_refuses_a_bad_output_rate():
    from gf3_audio_modem_amd.OFDM import transmitter
    for bad in ("44100", 1000, float("nan"), True):
        tx = transmitter("A2", no_pilots=2, packet_length=4)
        tx.output_rate = bad
        with pytest.raises(ValueError, match="output_rate"):
            tx.transmit(np.zeros(100, dtype=np.int64))
    tx = transmitter("A2", no_pilots=2, packet_length=4)
    tx.output_rate, tx.rate_taps = 44100, 12
    with pytest.raises(ValueError, match="rate_taps"):
        tx.transmit(np.zeros(100, dtype=np.int64))


def test_live_receiver_takes_the_rate_from_the_receiver():
    from gf3_audio_modem_amd.live import LiveReceiver
    live = LiveReceiver(rx_of(input_rate=44100))
    assert live.rate == (44100.0, 32) and live.r == 44100.0 / 48000 and live.eng is None
    assert LiveReceiver(rx_of()).rate is None and LiveReceiver(rx_of()).r == 1.0
    with pytest.raises(ValueError, match="input_rate"):
        LiveReceiver(rx_of(input_rate=1e6))
    assert math.floor(26000 * live.r) == 23887
