"""Sampling-clock correction, host side (no GPU): the library's coefficient table against the NumPy restatement
(tests/resample_ref.py), the restated interpolator against exact off-grid sinusoids, the whole chain -- estimate from the
slope, resample, demodulate -- on the oracle with an exactly synthesised clock offset, and the façade's refusals."""
import ctypes as C

import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import resample_ref as RR


# ---- 1. the table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [16, 32])
def test_library_table_equals_the_restatement(T):
    from gf3_audio_modem_amd import _lib
    lib = _lib.load()
    h = np.full((RR.L + 1, 2 * T), np.nan)
    assert lib.gf3_resample_coefficients(T, h.ctypes.data_as(_lib.c_double_p)) == 0
    ref = RR.table(T)
    err = float(np.abs(h - ref).max())
    print(f"T = {T}: largest |library - restatement| {err:.3e}; sum |c| at most {np.abs(ref).sum(axis=1).max():.4f}")
    assert err <= 1e-14
    impulse = np.zeros(2 * T)
    impulse[T - 1] = 1.0
    assert np.array_equal(h[0], impulse) and np.array_equal(ref[0], impulse)
    assert np.array_equal(h[RR.L], np.roll(impulse, 1)) and np.array_equal(ref[RR.L], np.roll(impulse, 1))
    assert np.abs(ref).sum(axis=1).max() < 4.0              # (what the GPU test's tolerance assumes)


def test_library_table_refuses_other_tap_counts():
    from gf3_audio_modem_amd import _lib
    lib = _lib.load()
    h = np.zeros((RR.L + 1) * 64)
    for bad in (8, 0, -16, 24, 64):
        assert lib.gf3_resample_coefficients(bad, h.ctypes.data_as(_lib.c_double_p)) == _lib.GF3_EINVAL
        assert b"gf3_resample_coefficients" in lib.gf3_last_error(None)
    assert lib.gf3_resample_coefficients(16, None) == _lib.GF3_EINVAL
    assert not h.any()


# ---- 2. the interpolator against exact sinusoids --------------------------------------------------------------------
def sinusoid_error_db(T, eps, w):
    """Worst error in dB (amplitude 1) of the restated resampler on cos(w pi n + 0.3), a body of 6000 samples 100 samples
    into the stream, against the same cosine at the times j / (1 + eps)."""
    lead, n_body = 100, 6000
    n = np.arange(lead + n_body + 100)
    x = np.cos(w * np.pi * (n - lead) + 0.3)
    _, raw, status = RR.resample_rows(x, [lead], n_body, eps, T)
    assert status.tolist() == [0]
    exact = np.cos(w * np.pi * (np.arange(n_body) / (1.0 + eps)) + 0.3)
    return 20.0 * np.log10(np.abs(raw[0] - exact).max())


@pytest.mark.parametrize("T,bar,band", [(16, -95.0, (0.25, 0.49, 0.74)), (32, -100.0, (0.25, 0.49, 0.74, 0.85))])
def test_restatement_against_exact_sinusoids(T, bar, band):
    """Measured: T = 16: -100.9 dB (0.74 pi at 1000 ppm, the worst of its band; -112 dB and better below 0.5 pi), T = 32:
    -106.3 dB (0.74 pi at 1000 ppm; -107.9 dB at 0.85 pi); every figure is printed."""
    worst = -np.inf
    for eps in (50e-6, 1e-3):
        for w in band:
            db = sinusoid_error_db(T, eps, w)
            print(f"T = {T}, eps = {eps:g}, {w} pi: {db:.1f} dB")
            worst = max(worst, db)
    print(f"T = {T}: worst {worst:.1f} dB (bar {bar} dB)")
    assert worst <= bar


def test_beyond_the_band_the_error_is_what_the_documents_say():
    """Not a bar: the band limits README and DESIGN state (T = 16: about -40 dB at 0.85 pi, T = 32: about -20 dB at 0.95 pi)."""
    a, b = sinusoid_error_db(16, 1e-3, 0.85), sinusoid_error_db(32, 1e-3, 0.95)
    print(f"T = 16 at 0.85 pi: {a:.1f} dB; T = 32 at 0.95 pi: {b:.1f} dB")
    assert -60.0 < a < -30.0 and -35.0 < b < -10.0


def test_zero_offset_status_and_storage():
    rng = np.random.default_rng(3)
    x = rng.normal(size=700)
    rows, raw, status = RR.resample_rows(x, [0, 100, 201, -1], 500, [0.0, np.nan, 3e-3, 0.0], 16)
    assert status.tolist() == [0, 2, 3, 1]
    assert np.array_equal(rows[0], x[:500]) and np.array_equal(rows[1], x[100:600]) and not rows[2].any() and not rows[3].any()
    assert RR.status_of([200, 201], [2e-3, -2.0000001e-3], 500, 700).tolist() == [0, 3]
    assert RR.to_storage(np.array([0.5, 1.5, 2.5, -0.5, 300.0, -7.0]), np.uint8).tolist() == [0, 2, 2, 0, 255, 0]
    assert RR.to_storage(np.array([1e9, -1e9, 2.5]), np.int16).tolist() == [32767, -32768, 2]
    assert RR.to_storage(np.array([0.1]), np.float32)[0] == np.float32(0.1)


# ---- 3. the whole chain on the oracle -------------------------------------------------------------------------------
def chain_params():
    rng = np.random.default_rng(5)
    pts, bt = orc.qpsk_table()
    return orc.RxParams(N=1024, CP=128, P=2, D=8, lo=25, hi=375, const_points=pts, const_bits=bt,
                        known_bits=rng.integers(0, 2, size=1022).astype(np.uint8), fit_lo=100, fit_hi=300)


@pytest.fixture(scope="module")
def undrifted():
    """The packet without an offset: bits, filler, the stream, the noise (40 dB under the body), its demodulation without and
    with the noise -> the reference symbols and the noise floor of the error vector."""
    p = chain_params()
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 2, size=p.D * p.C * p.mu).astype(np.uint8)
    fill = orc.qpsk_table()[0][rng.integers(0, 4, size=p.K - p.C)]
    lead, tail = 300, 300
    clean = orc.tx_stream(bits, fill, p, lead=lead, tail=tail)
    start = lead + p.Lc
    sigma = float(np.sqrt(np.mean(clean[start: start + p.M * p.S] ** 2))) / 100.0
    noise = np.random.default_rng(7).normal(0.0, sigma, len(clean) + 2 * p.frame_len // 100 + 64)
    ref = orc.demod_frames(clean, np.array([start]), p)["eq"]
    noisy = orc.demod_frames(clean + noise[: len(clean)], np.array([start]), p)
    floor = evm_db(noisy["eq"], ref)
    assert np.array_equal(noisy["bits"], bits)
    return dict(p=p, bits=bits, fill=fill, lead=lead, tail=tail, noise=noise, ref=ref, floor=floor)


def evm_db(eq, ref):
    return 10.0 * np.log10(np.mean(np.abs(eq - ref) ** 2) / np.mean(np.abs(ref) ** 2))


@pytest.mark.parametrize("ppm", [200.0, -200.0, 1000.0])
def test_chain_on_the_oracle(undrifted, ppm):
    """The packet's start is the last receiver sample not after the body's first instant, floor((lead + Lc) / (1 + eps)): what
    a sync without error gives.  The subject is the estimate and the resampler, not the chirp search -- whose answer is
    asserted to lie within 3 samples and printed: at 1000 ppm the chirp itself is stretched by 5.8 samples and the oracle's
    search lands one sample late, inside the next symbol, which costs every symbol -28 dB of inter-symbol interference
    before and after any resampling (the reference leaves no timing margin).
    Measured (printed): estimates 0.11 %, 0.02 % and 0.76 % off; the error vector -13.7 -> -37.6 dB, -14.0 -> -37.5 dB and
    7.9 -> -36.6 dB against a -38.6 dB floor; at 1000 ppm 21.3 % bit errors before and none after."""
    u = undrifted
    p, eps = u["p"], ppm * 1e-6
    r = RR.drifted_stream(u["bits"], u["fill"], p, eps, lead=u["lead"], tail=u["tail"])
    r = r + u["noise"][: len(r)]
    true = (u["lead"] + p.Lc) / (1.0 + eps)
    found = orc.frame_starts(orc.chirp_method(r, p))
    assert len(found) == 1 and abs(found[0] - true) < 3
    starts = np.array([int(np.floor(true))])
    print(f"{ppm:+.0f} ppm: the body starts at {true:.2f}, taken from {starts[0]}; the chirp search says {found[0]}")
    first = orc.demod_frames(r, starts, p)
    est = float(RR.clock_offset(first["slope"], p)[0])
    rows, _, status = RR.resample_rows(r, starts, p.M * p.S, est, 16)
    assert status.tolist() == [0]
    second = orc.demod_frames(rows[0], np.array([0]), p)
    before, after = evm_db(first["eq"], u["ref"]), evm_db(second["eq"], u["ref"])
    ber = [float(np.mean(o["bits"] != u["bits"])) for o in (first, second)]
    print(f"{ppm:+.0f} ppm: estimate {est * 1e6:+.2f} ppm ({abs(est / eps - 1) * 100:.2f} % off); error vector {before:.1f} dB -> "
          f"{after:.1f} dB, floor {u['floor']:.1f} dB; bit errors {ber[0] * 100:.1f} % -> {ber[1] * 100:.1f} %")
    assert abs(est / eps - 1.0) <= 0.01
    assert before - after >= 15.0 and after <= u["floor"] + 6.0
    if ppm == 1000.0:
        assert ber[0] > 0.10 and ber[1] == 0.0


def test_drifted_stream_without_an_offset_is_the_stream():
    p = chain_params()
    rng = np.random.default_rng(8)
    bits = rng.integers(0, 2, size=p.D * p.C * p.mu).astype(np.uint8)
    fill = orc.qpsk_table()[0][rng.integers(0, 4, size=p.K - p.C)]
    a, b = orc.tx_stream(bits, fill, p, lead=11, tail=5), RR.drifted_stream(bits, fill, p, 0.0, lead=11, tail=5)
    assert a.shape == b.shape and np.abs(a - b).max() < 1e-11
    np.testing.assert_allclose(RR.clock_offset([2 * np.pi], p), [p.N / ((p.P + p.D) * p.S)], rtol=1e-15)


# ---- 4. the façade's refusals ---------------------------------------------------------------------------------------
def test_facade_defaults_and_refusals_before_any_gpu_work():
    from gf3_audio_modem_amd.coding import check_clock
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2", encoding="None")
    assert rx.clock_correction is None and rx.clock_taps == 32
    assert rx.last_clock_ppm is None and rx.last_clock_ppm_packets is None
    assert check_clock(None, 5) is None and check_clock("auto", 32) == ("auto", 16) and check_clock(-150, 64) == (-150.0, 32)
    assert check_clock(np.float64(2000.0), 32) == (2000.0, 16)
    for bad in ("on", "AUTO", "", np.nan, np.inf, -np.inf, 2000.5, -3000, True, [1.0], (1,)):
        rx.clock_correction = bad
        with pytest.raises(ValueError, match="clock_correction"):     # (no engine exists yet: nothing touched the GPU)
            rx.receive(np.zeros(10))
        with pytest.raises(ValueError, match="clock_correction"):
            rx.receive_diversity([np.zeros(10)])
    for bad in (16, 48, 128, 32.5, None, "32", True):
        rx.clock_correction, rx.clock_taps = "auto", bad
        with pytest.raises(ValueError, match="clock_taps"):
            rx.receive(np.zeros(10))
        rx.clock_correction = 50.0
        with pytest.raises(ValueError, match="clock_taps"):
            rx.receive_diversity([np.zeros(10)])
    assert not rx._engines


def test_abi_names_are_declared_and_bound():
    import os
    import re
    from gf3_audio_modem_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = set(re.findall(r"\b(gf3_[a-z_]+)\s*\(", open(os.path.join(root, "include", "gf3rx.h")).read()))
    assert {"gf3_resample_frames", "gf3_resample_coefficients"} <= names
    assert len(_lib._SIGS["gf3_resample_frames"][1]) == 10 and _lib._SIGS["gf3_resample_coefficients"][1] == [C.c_int32, _lib.c_double_p]
    unit = os.path.join(root, "gf3_audio_modem_amd", "csrc", "gf3rx_resample.hip")
    assert unit in build.SRC and "gf3_resample_frames" in open(unit).read()
    shared = open(os.path.join(root, "gf3_audio_modem_amd", "csrc", "gf3rx_storage.h")).read()
    assert "to_storage" in shared and "to_storage<DT_F32>(double" not in open(os.path.join(root, "gf3_audio_modem_amd", "csrc", "gf3rx_blank.hip")).read()
