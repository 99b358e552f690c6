"""Receive windowing on the GPU: gf3_window_frames against the NumPy restatement (tests/window_ref.py) at the smallest shapes
at which the kernel can go wrong, its refusals, and `receive_window` end to end through the façade under the interferer of
tests/test_window_cpu.py, which settles the tone level.  The guard-band rows are in tests/test_bounds_window_gpu.py.

Shape of the kernel tests: tests/test_resample_gpu.py's engine, N = 1024, CP = 56, P = 1, D = 2 -- a symbol has S = 1080 samples,
no multiple of 16 bytes' worth of elements in uint8 storage, four symbols per packet, three packets that start at odd samples (3, 4340, 8689), so that input and output share their offset within 16 bytes
in some symbols and not in others; ramps of 1, 2, 3 (inside one vector), 55 and 56 = CP samples.  And the longest prefix of
the standard, N = 4096, CP = 1184 = L, with a packet that starts before the samples and one that runs past them.

Tolerances.  The reference is the restatement evaluated in np.longdouble, whose own rounding is 2^-11 of the kernel's.  A
ramp output a (1 - r) + b r takes four rounded fp64 operations of which a contraction removes one: |got - ref| <= 4 x 2^-53
(|a| + |b|); float32 storage adds one float32 ulp of the result; every sample outside the ramps is the input's own bytes.
Integer storage: no reference value lies within 1e-9 of a half-integer (asserted first), then equality.  Report: every term
is non-negative, so rtol (L + 4) 2^-53 in the float storages; the integer storages' sums are exact in fp64: equality."""
import functools

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import window_ref as WR
from tests.test_live_gpu import quiet
from tests.test_resample_gpu import N_BODY, N_IN, STARTS, engine_of, longest_prefix_case, samples
from tests.test_window_cpu import LEVEL_DB, PACKETS

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
N, CP, M = 1024, 56, 4
S = N + CP


def held(out, report, x, starts, n, cp, m, L):
    """The engine's rows and report against the restatement, at the tolerances above -> the largest error over its bound"""
    x = np.asarray(x)
    s = n + cp
    rows, raw, status, rep = WR.window_rows(x, starts, n, cp, m, L, work=np.longdouble)
    F = len(starts)
    ok = status == 0
    out = out.reshape(F, m, s)
    raw, rows = raw.reshape(F, m, s), rows.reshape(F, m, s)
    assert not out[~ok].any()                                # a ragged packet's row is zeros
    assert np.isnan(report[~ok]).all()
    src = np.stack([x[st: st + m * s].reshape(m, s) if good else np.zeros((m, s), x.dtype) for st, good in zip(starts, ok)])
    assert np.array_equal(out[ok][:, :, : s - L].view(np.uint8), src[ok][:, :, : s - L].view(np.uint8))     # copied as they are
    worst = 0.0
    if x.dtype.kind == "f":
        a, b = np.abs(src[..., s - L:].astype(np.float64)), np.abs(src[..., cp - L: cp].astype(np.float64))
        bound = 4 * U * (a + b)
        if x.dtype == np.float32:
            bound = bound + np.spacing(np.abs(raw[..., s - L:]).astype(np.float32)).astype(np.float64)
        err = np.abs(out[..., s - L:].astype(np.longdouble) - raw[..., s - L:]).astype(np.float64)
        assert (err[ok] <= bound[ok]).all(), float((err[ok] / np.maximum(bound[ok], 1e-300)).max())
        worst = float((err[ok] / np.maximum(bound[ok], 1e-300)).max())
        rerr = np.abs(report[ok].astype(np.longdouble) - rep[ok]).astype(np.float64)
        assert (rerr <= (L + 4) * U * rep[ok].astype(np.float64)).all()
    else:
        frac = np.abs(raw[ok] - np.floor(raw[ok])).astype(np.float64)
        assert (np.abs(frac - 0.5) > 1e-9).all()             # nothing for the rounding to disagree about
        assert np.array_equal(out[ok], rows[ok])
        assert np.array_equal(report[ok], rep[ok].astype(np.float64))
    return status, worst


@pytest.mark.parametrize("L", [1, 2, 3, 55, 56])
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int16, np.uint8])
def test_kernel_against_the_restatement(dtype, L):
    eng = engine_of(dtype)
    assert (eng.cfg.N, eng.cfg.CP, eng.cfg.M) == (N, CP, M)
    x = samples(dtype)
    starts = STARTS[:3]
    if x.dtype.kind != "f" and L % 2:
        # the raised cosine of an odd L is 0.5 exactly at its centre, where the output is (a + b) / 2: the seeded integers are
        # moved by one where a + b is odd, so that no reference value is a half-integer (`held` asserts it)
        x = x.copy()
        for st in starts:
            for m in range(M):
                a, b = st + m * S + S - L + (L - 1) // 2, st + m * S + CP - L + (L - 1) // 2
                x[a] += (int(x[a]) + int(x[b])) % 2
    xt = torch.from_numpy(x).cuda()
    out, off, st, report = eng.window_frames(xt, starts, L)
    assert out.dtype == xt.dtype and tuple(out.shape) == (3, N_BODY) and out.is_contiguous()
    assert off.dtype == torch.int64 and off.tolist() == [0, N_BODY, 2 * N_BODY]
    assert st.dtype == torch.int32 and st.tolist() == [0, 0, 0]
    assert report.dtype == torch.float64 and tuple(report.shape) == (3, M, 2)
    assert np.array_equal(xt.cpu().numpy().view(np.uint8), x.view(np.uint8))          # the input is not written
    _, worst = held(out.cpu().numpy(), report.cpu().numpy(), x, starts, N, CP, M, L)
    print(f"{np.dtype(dtype).name} L {L}: largest error / bound {worst:.3f}")
    # the same bytes on a second call
    again = eng.window_frames(xt, starts, L)
    for a, b in zip((out, off, st, report), again):
        assert a is not b and np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int16])
def test_kernel_at_the_longest_prefix(dtype):
    """N = 4096, CP = L = 1184, P = 2, D = 2: the ramp is a fifth of the symbol and reaches back to the symbol's first sample.
    Four packets: one that starts before the samples, two inside them, one that runs a sample past their end."""
    eng, x, _, body = longest_prefix_case(dtype)
    starts = np.array([-1, 3, 3 + body + 17, len(x) - body + 1])
    xt = torch.from_numpy(x).cuda()
    out, off, st, report = eng.window_frames(xt, starts, 1184)
    assert tuple(out.shape) == (4, body) and off.tolist() == [0, body, 2 * body, 3 * body] and st.tolist() == [1, 0, 0, 1]
    status, worst = held(out.cpu().numpy(), report.cpu().numpy(), x, starts, 4096, 1184, 6, 1184)
    assert status.tolist() == [1, 0, 0, 1]
    print(f"longest prefix, {np.dtype(dtype).name}: largest error / bound {worst:.3f}")


def test_nonfinite_samples_stay_where_they_enter():
    """A NaN in symbol 1's ramp reaches that one output; an Inf in symbol 2's folded stretch reaches its own copy and the one
    ramp output it is folded into; an Inf outside both stretches is copied.  The report: symbols 1 and 2 NaN, symbols 0 and 3 and
    the other packets as without the plants."""
    eng = engine_of(np.float64)
    x = samples(np.float64)
    L = 5
    s0 = int(STARTS[1])
    clean = eng.window_frames(torch.from_numpy(x).cuda(), STARTS[:3], L)
    x = x.copy()
    x[s0 + 2 * S - 2] = np.nan
    x[s0 + 2 * S + CP - 1] = np.inf
    x[s0 + 7] = -np.inf
    out, _, st, report = eng.window_frames(torch.from_numpy(x).cuda(), STARTS[:3], L)
    out, report = out.cpu().numpy(), report.cpu().numpy()
    assert st.tolist() == [0, 0, 0]
    assert np.flatnonzero(~np.isfinite(out[1])).tolist() == [7, 2 * S - 2, 2 * S + CP - 1, 3 * S - 1]
    assert np.isnan(out[1, 2 * S - 2]) and out[1, 7] == -np.inf and out[1, 2 * S + CP - 1] == np.inf and out[1, 3 * S - 1] == np.inf
    assert np.isfinite(out[[0, 2]]).all()
    assert np.isnan(report[1, 1:3]).all() and np.isfinite(report[[0, 2]]).all() and np.isfinite(report[1, [0, 3]]).all()
    keep = np.ones(N_BODY, dtype=bool)
    keep[[7, 2 * S - 2, 2 * S + CP - 1, 3 * S - 1]] = False
    ref_out, ref_report = clean[0].cpu().numpy(), clean[3].cpu().numpy()
    assert np.array_equal(out[1, keep], ref_out[1, keep]) and np.array_equal(out[[0, 2]], ref_out[[0, 2]])
    assert np.array_equal(report[[0, 2]], ref_report[[0, 2]]) and np.array_equal(report[1, [0, 3]], ref_report[1, [0, 3]])
    held(out[[0, 2]], report[[0, 2]], x, STARTS[[0, 2]], N, CP, M, L)


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_the_clock_corrections_rows_are_an_input(dtype):
    """resample_frames' (rows, offsets) go in as (x, starts): the two stages chain, and the result is the restatement's on
    those rows."""
    eng = engine_of(dtype)
    xt = torch.from_numpy(samples(dtype)).cuda()
    rows, off, st = eng.resample_frames(xt, STARTS[:3], [50e-6, -50e-6, 0.0])
    assert not st.any()
    out, off2, st2, report = eng.window_frames(rows, off, 56)     # (an even L: no ramp value is 0.5, no half-integers)
    assert tuple(out.shape) == (3, N_BODY) and off2.tolist() == off.tolist() and st2.tolist() == [0, 0, 0]
    assert out.data_ptr() != rows.data_ptr()
    held(out.cpu().numpy(), report.cpu().numpy(), rows.cpu().numpy().reshape(-1), off.cpu().numpy(), N, CP, M, 56)
    o = eng.demod_frames(out, off2, want=("Hs", "status"))
    assert not o["status"].any()


def test_no_packets_an_own_buffer_and_refusals():
    from gf3_audio_modem_amd import _lib
    eng = engine_of(np.float64)
    x = samples(np.float64)
    xt = torch.from_numpy(x).cuda()
    rows, off, st, report = eng.window_frames(xt, torch.empty(0, dtype=torch.int64), 8)
    assert tuple(rows.shape) == (0, N_BODY) and off.numel() == 0 and st.numel() == 0 and tuple(report.shape) == (0, M, 2)
    mine = torch.full((2 * N_BODY,), 7.0, dtype=torch.float64, device="cuda")
    rows, _, _, report = eng.window_frames(xt, STARTS[:2], 8, out=mine)
    assert rows.data_ptr() == mine.data_ptr() and tuple(rows.shape) == (2, N_BODY)
    held(rows.cpu().numpy(), report.cpu().numpy(), x, STARTS[:2], N, CP, M, 8)
    for bad in (-1, CP + 1, 1.5, True, None, "8"):
        with pytest.raises(ValueError, match="receive_window must be an integer"):
            eng.window_frames(xt, STARTS, bad)
    with pytest.raises(ValueError, match="taper of 0 samples"):
        eng.window_frames(xt, STARTS, 0)
    with pytest.raises(ValueError, match="out"):
        eng.window_frames(xt, STARTS, 8, out=mine)
    lib, p = eng.lib, _lib.ptr
    off = torch.from_numpy(STARTS).cuda()
    ramp = torch.from_numpy(WR.ramp(8)).cuda()
    out = torch.full((4, N_BODY), 7.0, dtype=torch.float64, device="cuda")
    report = torch.full((4, M, 2), 7.0, dtype=torch.float64, device="cuda")
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    good = [eng._h, p(xt), xt.numel(), p(off), 4, p(ramp), 8, p(out), p(report), p(status), None]
    cases = [(at, None) for at in (0, 1, 3, 5, 7, 8, 9)] + [(4, -1), (2, -1), (6, 0), (6, -1), (6, CP + 1), (7, p(xt)), (4, 65536)]
    for at, value in cases:
        args = list(good)
        args[at] = value
        assert lib.gf3_window_frames(*args) == _lib.GF3_EINVAL, (at, value)
        assert b"gf3_window_frames" in lib.gf3_last_error(None)
    args = list(good)
    args[4], args[7] = 0, p(xt)                                    # refused even when there is nothing to do
    assert lib.gf3_window_frames(*args) == _lib.GF3_EINVAL
    args = [eng._h, None, 0, None, 0, None, CP, None, None, None, None]    # F = 0: no array needs an address
    assert lib.gf3_window_frames(*args) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (report == 7.0).all() and (status == 77).all()      # no refusal wrote anything
    assert lib.gf3_window_frames(*good) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 1] and N_IN - int(STARTS[3]) == N_BODY - 1
    held(out.cpu().numpy(), report.cpu().numpy(), x, STARTS, N, CP, M, 8)


# ---- end to end through the façade ----------------------------------------------------------------------------------
CODEWORDS = 29


def facade(**attrs):
    """Mode A2 with no_pilots = 4, packet_length = 8, "QCLDPC-1/2", the noise weights: the scenario of tests/test_window_cpu.py"""
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2", encoding="QCLDPC-1/2", no_pilots=4, packet_length=8)
    rx.llr_weighting = "noise"
    for k, v in attrs.items():
        setattr(rx, k, v)
    return rx


def oracle_params(rx):
    pts, bt = orc.qpsk_table()
    return orc.RxParams(N=4096, CP=224, P=4, D=8, lo=100, hi=1500, const_points=pts, const_bits=bt,
                        known_bits=np.asarray(rx.known_sequence, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def heard(kind):
    """Two packets of 29 codewords through `transmit` (kind "one") or `transmit_stbc` (kind "stbc": the speakers through
    window_ref.channel(5) and channel(6) into ONE microphone) and the scenario's channel, noiseless
    -> (payload, the recording, its RMS over the bodies)"""
    rx = facade(llr_weighting="csi") if kind == "stbc" else facade()
    p = oracle_params(rx)
    payload = np.random.default_rng(3).integers(0, 2, size=CODEWORDS * 768)
    np.random.seed(5)                                       # (the fill of the last packet, the filler of the unused carriers)
    tx = np.atleast_2d(quiet(rx.transmit_stbc if kind == "stbc" else rx.transmit, payload))
    assert rx.no_packets == PACKETS and tx.shape[1] == PACKETS * p.frame_len + p.Lc
    tx = np.concatenate([np.zeros((len(tx), WR.LEAD)), tx, np.zeros((len(tx), WR.TAIL))], axis=1)
    clean = sum(np.convolve(row, WR.channel(5 + i))[: tx.shape[1]] for i, row in enumerate(tx))
    return payload, clean, WR.body_rms(clean, p, PACKETS)


def expect_report(rx, shape):
    rep = rx.last_window_report
    assert set(rep) == {"taper", "mismatch_db"} and rep["taper"] == WR.TAPER
    assert rep["mismatch_db"].dtype == np.float64 and rep["mismatch_db"].shape == shape
    return rep["mismatch_db"]


def test_receive_under_the_tone_at_the_settled_level():
    """transmit -> 40 taps, 25 dB of white noise, the tone at LEVEL_DB -> receive: exact under receive_window = 128, failed
    codewords without it.  The mismatch the call reports is the restatement's on the same samples and starts."""
    payload, clean, rms = heard("one")
    r = WR.interfered(clean, rms, LEVEL_DB)
    rx = facade(receive_window=WR.TAPER)
    bits, Hs0, He0 = quiet(rx.receive, r)
    report = rx.last_decode_report
    db = expect_report(rx, (PACKETS,))
    p = oracle_params(rx)
    starts = orc.frame_starts(orc.chirp_method(r, p))
    want = WR.mismatch_db(WR.window_rows(r, starts, p.N, p.CP, p.M, WR.TAPER)[3])
    print(f"tone {LEVEL_DB:+.0f} dB, L = {WR.TAPER}: report {report}, mismatch {db} dB (restatement {want})")
    assert report["codewords"] == CODEWORDS and report["inner_failed"] == 0
    assert np.array_equal(bits[: len(payload)], payload)
    np.testing.assert_allclose(db, want, rtol=0, atol=1e-9)
    rx.receive_window = 0
    quiet(rx.receive, r)
    print(f"tone {LEVEL_DB:+.0f} dB, no window: report {rx.last_decode_report}")
    assert rx.last_window_report is None and rx.last_decode_report["inner_failed"] >= 1
    # the fused sample-to-LLR demodulator and the denoiser read the windowed rows too
    fused = facade(llr_weighting="csi", fused_llr=True, receive_window=WR.TAPER)
    quiet(fused.receive, r)
    np.testing.assert_allclose(expect_report(fused, (PACKETS,)), want, rtol=0, atol=1e-9)
    den = facade(channel_denoising=True, receive_window=WR.TAPER)
    quiet(den.receive, r)
    np.testing.assert_allclose(expect_report(den, (PACKETS,)), want, rtol=0, atol=1e-9)
    assert den.last_denoise_report.shape == (PACKETS, 2, 5)
    print(f"with the denoiser: report {den.last_decode_report}")


def test_receive_diversity_under_the_tone():
    payload, clean, rms = heard("one")
    rs = [WR.interfered(clean, rms, LEVEL_DB, seed=5), WR.interfered(clean, rms, LEVEL_DB, seed=6)]
    rx = facade(receive_window=WR.TAPER)
    bits, _, _ = quiet(rx.receive_diversity, rs)
    db = expect_report(rx, (2, PACKETS))
    print(f"two recordings, L = {WR.TAPER}: report {rx.last_decode_report}, mismatch {db.tolist()} dB")
    assert rx.last_decode_report["inner_failed"] == 0 and np.array_equal(bits[: len(payload)], payload)
    rx.receive_window = 0
    quiet(rx.receive_diversity, rs)
    print(f"two recordings, no window: report {rx.last_decode_report}")
    assert rx.last_window_report is None and rx.last_decode_report["inner_failed"] >= 1


def test_receive_stbc_under_the_tone_from_one_microphone():
    """The space-time code into one microphone, under the pilot-measured weights (the two-speaker calls' form of the noise
    weights: the notch the window leaves must be marked by something).  The advance of 48 samples, the 40 taps and the
    128 of the ramp fit the prefix of 224."""
    payload, clean, rms = heard("stbc")
    r = WR.interfered(clean, rms, LEVEL_DB)
    rx = facade(llr_weighting="csi", joint_weighting="noise", receive_window=WR.TAPER)
    bits, _, _ = quiet(rx.receive_stbc, [r])
    db = expect_report(rx, (1, PACKETS))
    print(f"space-time code, L = {WR.TAPER}: report {rx.last_decode_report}, mismatch {db.tolist()} dB")
    assert rx.last_decode_report["inner_failed"] == 0 and np.array_equal(bits[: len(payload)], payload)
    rx.receive_window = 0
    quiet(rx.receive_stbc, [r])
    print(f"space-time code, no window: report {rx.last_decode_report}")
    assert rx.last_window_report is None and rx.last_decode_report["inner_failed"] >= 1
    with pytest.raises(ValueError, match=r"mimo_advance \+ receive_window = 48 \+ 177"):
        rx.receive_window = 177
        quiet(rx.receive_stbc, [r])


def test_live_receiver_under_the_tone():
    """The stream fed in two blocks.  Under the tone the chirp's correlation coefficient is 0.19 (the tone's power is 40 times
    the signal's) and nothing else in the stream reaches 0.003: detect_threshold = 0.1."""
    from gf3_audio_modem_amd import LiveReceiver
    payload, clean, rms = heard("one")
    r = WR.interfered(clean, rms, LEVEL_DB)
    for taper in (WR.TAPER, 0):
        rx = facade(receive_window=taper, detect_threshold=0.1)
        live = LiveReceiver(rx)
        got = live.feed(r[: len(r) // 2]) + live.feed(r[len(r) // 2:]) + live.flush()
        assert len(got) == 1 and got[0].no_packets == PACKETS, live.events
        print(f"live, L = {taper}: report {got[0].decode_report}")
        if taper:
            assert got[0].decode_report["inner_failed"] == 0 and np.array_equal(got[0].bits[: len(payload)], payload)
            expect_report(rx, (PACKETS,))
        else:
            assert got[0].decode_report["inner_failed"] >= 1 and rx.last_window_report is None


def test_a_clean_packet_is_left_as_it_is():
    """Noiseless, through the 40 taps (shorter than CP - L = 96): the same bits and, within 1e-9 of the largest, the same Hs
    with and without the window; the two stretches the window blends agree to rounding."""
    payload, clean, _ = heard("one")
    rx = facade()
    plain = quiet(rx.receive, clean)
    assert rx.last_window_report is None
    rx.receive_window = WR.TAPER
    windowed = quiet(rx.receive, clean)
    db = expect_report(rx, (PACKETS,))
    print(f"noiseless: mismatch {db.tolist()} dB, largest change of Hs {np.abs(windowed[1] - plain[1]).max() / np.abs(plain[1]).max():.2e}")
    assert np.array_equal(windowed[0], plain[0]) and np.array_equal(plain[0][: len(payload)], payload)
    assert np.abs(windowed[1] - plain[1]).max() <= 1e-9 * np.abs(plain[1]).max()
    assert (db < -250.0).all()
