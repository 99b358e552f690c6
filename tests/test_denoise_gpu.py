"""The delay-domain pilot denoiser on the GPU: denoise_kernel against its NumPy restatement (tests/denoise_ref.py),
gf3_demod_frames_dn against the oracle fed with the restatement's pilot sums, the untouched two-phase form against digests
recorded before the feature, the façade end to end, and the real recording.

Tolerance of psum'.  The kernel runs four fp64 transforms; one is held to 1e-12 of the row's maximum (test_rfft_batch), so
|psum' - restatement| <= 4e-12 max|row|.  The keep decisions are compared as integers: the test first asserts, with the
restatement alone, that no tap of its inputs lies within 1e-6 (relative) of the threshold, six orders above the rounding
of either side.  v to 1e-10 relative (two summation orders of ~1e4 .. 1e5 squares: ~1e-14).  Measured on the MI355X at
N = 2048 and 4096 (all four storages, P = 2, 3, 9): |psum' - restatement| / max|row| 6.0e-16 .. 1.7e-15."""
import dataclasses
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import denoise_ref as DR
from tests.util import GOLD, engine_for, load, modeA2_params, params_of

pytestmark = pytest.mark.gpu
TORCH_OF = {"float64": torch.float64, "float32": torch.float32, "int16": torch.int16, "uint8": torch.uint8}
KNOWN = np.random.default_rng(1).integers(0, 2, size=2 * 511)
CASES = {}


def case(N, P, dtype):
    """Input, restatement and engine of one kernel case: computed once, shared, left unchanged."""
    key = (N, P, dtype)
    if key not in CASES:
        p, x, starts = DR.kernel_case(N, P, dtype, seed=N + P)
        ref = DR.denoise_frames(x, starts, p.N, p.CP, p.P, p.D, p.known_symbols())
        CASES[key] = (p, x, starts, ref, engine_for(p, in_dtype=TORCH_OF[dtype], Lc=p.S))
    return CASES[key]


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("P", [2, 3, 9])
@pytest.mark.parametrize("dtype", ["float64", "float32", "int16", "uint8"])
@pytest.mark.parametrize("N", [1024, 2048, 4096, 8192])                # every denoise_kernel<NC, DT> of the dispatch
def test_kernel_against_the_restatement(N, dtype, P):
    p, x, starts, (want, rep, plain, margin), eng = case(N, P, dtype)
    print(f"N {N} {dtype} P {P}: nearest tap to the threshold {margin:.1e}")
    assert margin >= 1e-6
    xt = torch.from_numpy(x).cuda()
    psum, report = eng.denoise_pilots(xt, starts)
    assert psum.dtype == torch.float64 and tuple(psum.shape) == (3, 2, N) and tuple(report.shape) == (3, 2, 5)
    got, grep = psum.cpu().numpy(), report.cpu().numpy()
    assert same_bytes(xt.cpu().numpy(), x)                           # the samples are not written
    np.testing.assert_array_equal(grep[:, :, 1:], rep[:, :, 1:])     # kept, post, pre, applied: the same decisions
    finite = np.isfinite(rep[:, :, 0])
    assert np.array_equal(np.isnan(grep[:, :, 0]), np.isnan(rep[:, :, 0]))
    np.testing.assert_allclose(grep[:, :, 0][finite], rep[:, :, 0][finite], rtol=1e-10, atol=0.0)
    worst = 0.0
    for f in range(3):
        for side in range(2):
            if rep[f, side, 4]:
                err = float(np.abs(got[f, side] - want[f, side]).max() / np.abs(want[f, side]).max())
                worst = max(worst, err)
            else:                                                    # pass-through: pilot_sum's row, bit for bit
                assert np.array_equal(got[f, side], plain[f, side], equal_nan=True)
                ok = ~np.isnan(plain[f, side])
                assert same_bytes(got[f, side][ok], plain[f, side][ok])
    print(f"N {N} {dtype} P {P}: largest |psum' - restatement| / max|row| = {worst:.2e} (bound 4e-12)")
    assert worst <= 4e-12
    assert rep[2, :, 4].tolist() == [0, 0] and not got[2].any()      # the ragged packet: zero rows, left alone
    if np.dtype(dtype).kind == "f":
        assert np.isnan(rep[0, 0, 0]) and rep[0, 0, 4] == 0 and rep[0, 1, 4] == 1      # the NaN sits in a start pilot
    again = eng.denoise_pilots(xt, starts)
    assert same_bytes(again[0].cpu().numpy(), got) and same_bytes(again[1].cpu().numpy(), grep)


def test_noiseless_rows_pass_through_and_refusals():
    """Identical pilot repeats: v = 0, every tap is kept, more than N/4 -> the row is pilot_sum's.  The ABI's refusals."""
    from gf3_audio_modem_amd import _lib
    p, x, starts, _, eng = case(1024, 2, "float64")
    y = np.array(x)
    for f in range(2):
        for side in range(2):
            a = starts[f] + side * (p.P + p.D) * p.S
            y[a + p.S: a + 2 * p.S] = y[a: a + p.S]
    y = np.nan_to_num(y)
    want, rep, plain, _ = DR.denoise_frames(y, starts, p.N, p.CP, p.P, p.D, p.known_symbols())
    assert rep[:2, :, 0].tolist() == [[0, 0]] * 2 and (rep[:2, :, 1] > p.N // 4).all() and not rep[:, :, 4].any()
    yt = torch.from_numpy(y).cuda()
    psum, report = eng.denoise_pilots(yt, starts)
    np.testing.assert_array_equal(report.cpu().numpy(), rep)
    assert same_bytes(psum.cpu().numpy(), plain)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "9", None):
        with pytest.raises(ValueError, match="denoising threshold"):
            eng.denoise_pilots(yt, starts, threshold=bad)
        with pytest.raises(ValueError, match="denoising threshold"):
            eng.demod_frames(yt, starts, denoise=bad if bad is not None else "x")
    with pytest.raises(ValueError, match="two-phase"):
        eng.demod_frames(yt, starts, denoise=9.0, split=False)
    with pytest.raises(ValueError, match="two-phase"):
        eng.demod_frames(yt, starts, denoise=9.0, precision="screen")
    empty = eng.demod_frames(yt, torch.empty(0, dtype=torch.int64), denoise=9.0)
    assert tuple(empty["denoise_report"].shape) == (0, 2, 5) and eng.denoise_pilots(yt, [])[0].numel() == 0
    lib, ptr = eng.lib, _lib.ptr
    off = torch.from_numpy(starts).cuda()
    out = torch.full((3, 2, p.N), 7.0, dtype=torch.float64, device="cuda")
    bits = torch.zeros((3, eng.bytes_per_frame), dtype=torch.uint8, device="cuda")
    work = torch.zeros(int(lib.gf3_demod_workspace_bytes(eng._h, 3)), dtype=torch.uint8, device="cuda")
    for thr in (0.0, -3.0, float("nan"), float("inf")):
        assert lib.gf3_denoise_pilots(eng._h, ptr(yt), yt.numel(), ptr(off), 3, thr, ptr(out), None, None) == _lib.GF3_EINVAL
        assert b"gf3_denoise_pilots" in lib.gf3_last_error(None)
        assert lib.gf3_demod_frames_dn(eng._h, ptr(yt), yt.numel(), ptr(off), 3, ptr(bits), None, None, None, None, None, None,
                                       ptr(work), thr, None, None) == _lib.GF3_EINVAL
        assert b"gf3_demod_frames_dn" in lib.gf3_last_error(None)
    assert lib.gf3_demod_frames_dn(eng._h, ptr(yt), yt.numel(), ptr(off), 3, ptr(bits), None, None, None, None, None, None,
                                   None, 9.0, None, None) == _lib.GF3_EINVAL
    assert b"workspace" in lib.gf3_last_error(None)
    assert lib.gf3_denoise_pilots(eng._h, ptr(yt), yt.numel(), ptr(off), 3, 9.0, None, None, None) == _lib.GF3_EINVAL
    one = engine_for(dataclasses.replace(p, P=1), Lc=p.S)            # P = 1: no repeats to measure the noise from
    assert lib.gf3_denoise_pilots(one._h, ptr(yt), yt.numel(), ptr(off), 3, 9.0, ptr(out), None, None) == _lib.GF3_EINVAL
    assert b"P >= 2" in lib.gf3_last_error(None)
    assert lib.gf3_demod_frames_dn(one._h, ptr(yt), yt.numel(), ptr(off), 3, ptr(bits), None, None, None, None, None, None,
                                   ptr(work), 9.0, None, None) == _lib.GF3_EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                        # no refusal wrote anything


# ---- gf3_demod_frames_dn against the oracle ---------------------------------------------------------------------------
def stored(r, storage):
    """The stream in its storage type (int16: scaled to +-20000 at the largest sample)."""
    if storage == "int16":
        return np.rint(r * (20000.0 / np.abs(r).max())).astype(np.int16)
    return r


def oracle_denoised(x, starts, p, tau=9.0):
    """oracle.equalise on the data spectra and ONE pilot row per side, rfft(psum')[1 .. K] / P of the restatement."""
    psum, rep, _, margin = DR.denoise_frames(x, starts, p.N, p.CP, p.P, p.D, p.known_symbols(), tau)
    X = orc.demod_fft(orc.gather_frames(x, starts, p).astype(np.float64), p)
    data = orc.split_pilots(X, p)[0]
    rows = np.fft.rfft(psum, axis=-1)[:, :, 1:p.K + 1] / p.P
    eq, Hs, He, Hest, slope = orc.equalise(data, rows[:, 0:1], rows[:, 1:2], p)
    eq = eq[:, p.data_carriers - 1]
    return dict(eq=eq, Hs=Hs, He=He, Hest=Hest, slope=slope, bits=orc.demap_hard(eq, p)[0].reshape(-1), report=rep, margin=margin)


def off_ties(eq, tol=1e-9):
    """QPSK decisions that rounding cannot turn: both parts of the symbol away from zero."""
    return np.repeat(((np.abs(eq.real) > tol) & (np.abs(eq.imag) > tol)).reshape(-1), 2)


@pytest.mark.parametrize("storage", ["float64", "int16"])
def test_demod_frames_dn_against_the_oracle(storage):
    p = DR.small_params(KNOWN)
    r, starts, _ = DR.noisy_stream(p, seed=0)
    x = stored(r, storage)
    ref = oracle_denoised(x, starts, p)
    assert ref["margin"] >= 1e-6 and ref["report"][:, :, 4].all()
    eng = engine_for(p, in_dtype=TORCH_OF[storage])
    xt = torch.from_numpy(x).cuda()
    o = eng.demod_frames(xt, starts, want=("eq", "Hs", "He", "slope", "Hest", "status"), denoise=9.0)
    alone = eng.denoise_pilots(xt, starts)[1]
    assert torch.equal(o["denoise_report"], alone) and int(o["status"].item()) == 0
    np.testing.assert_array_equal(alone.cpu().numpy()[:, :, 1:], ref["report"][:, :, 1:])
    figures = {}
    for k in ("Hs", "He", "eq", "Hest"):
        figures[k] = float(np.abs(o[k].cpu().numpy().reshape(ref[k].shape) - ref[k]).max() / np.abs(ref[k]).max())
    figures["slope"] = float(np.abs(o["slope"].cpu().numpy() - ref["slope"]).max())
    print(f"{storage}: largest differences from the oracle {figures}")
    assert figures["Hs"] <= 1e-11 and figures["He"] <= 1e-11 and figures["slope"] <= 1e-11
    assert figures["eq"] <= 1e-12 and figures["Hest"] <= 1e-12
    bits = eng.unpack_bits(o["bits"]).cpu().numpy()
    sure = off_ties(ref["eq"])
    assert sure.mean() > 0.999 and np.array_equal(bits[sure], ref["bits"][sure])
    lean = eng.demod_frames(xt, starts, denoise=9.0)                 # no dumps: Hs / He / slope live in the workspace
    assert torch.equal(lean["bits"], o["bits"]) and torch.equal(lean["denoise_report"], alone)
    plain = eng.demod_frames(xt, starts, want=("Hs",), split=True)
    assert "denoise_report" not in plain and not torch.equal(plain["Hs"], o["Hs"])


# ---- the standard's longest prefix: mode C3 --------------------------------------------------------------------------
_C3 = {}


def c3_case():
    """The reference-made fixture of mode C3 (N = 4096, CP = 1184, P = 2, D = 2, carriers 100 .. 999; int16 samples): its
    channel's last echo lies 0.8 CP = 947 samples behind the direct path, a delay no prefix of the A column holds.
    -> (p, x int16, starts, restatement of the kernel, the oracle on the restatement's pilot sums); made once."""
    if not _C3:
        g = load("g12_mode_C3")
        p = params_of(g)
        assert (p.N, p.CP, p.P, p.D, p.lo, p.hi) == (4096, 1184, 2, 2, 100, 1000) and int(np.flatnonzero(g["channel"])[-1]) == 947
        x, starts = g["r"], np.asarray(g["peaks"][:-1]) + 2
        _C3["case"] = (p, x, starts, DR.denoise_frames(x, starts, p.N, p.CP, p.P, p.D, p.known_symbols()), oracle_denoised(x, starts, p))
    return _C3["case"]


@pytest.mark.parametrize("storage", ["int16", "float32"])
def test_longest_prefix_kernel_and_demod_against_restatement_and_oracle(storage):
    """denoise_kernel and gf3_demod_frames_dn at S = 5280 (symbol offsets from CP = 1184), at the bars of
    test_kernel_against_the_restatement and test_demod_frames_dn_against_the_oracle; the echo at 947 samples is a kept tap."""
    p, x16, starts, (want, rep, plain, margin), ref = c3_case()
    assert margin >= 1e-6 and rep[:, :, 4].all() and (np.abs(rep[:, :, 2] - 947) <= 1).all()
    x = x16.astype(np.dtype(storage))                                # (the same values in either storage)
    eng = engine_for(p, in_dtype=TORCH_OF[storage])
    xt = torch.from_numpy(x).cuda()
    psum, report = eng.denoise_pilots(xt, starts)
    got, grep = psum.cpu().numpy(), report.cpu().numpy()
    assert same_bytes(xt.cpu().numpy(), x)
    np.testing.assert_array_equal(grep[:, :, 1:], rep[:, :, 1:])
    np.testing.assert_allclose(grep[:, :, 0], rep[:, :, 0], rtol=1e-10, atol=0.0)
    worst = max(float(np.abs(got[f, s] - want[f, s]).max() / np.abs(want[f, s]).max()) for f in range(len(starts)) for s in range(2))
    print(f"C3 {storage}: largest |psum' - restatement| / max|row| = {worst:.2e} (bound 4e-12)")
    assert worst <= 4e-12
    o = eng.demod_frames(xt, starts, want=("eq", "Hs", "He", "slope", "Hest", "status"), denoise=9.0)
    assert torch.equal(o["denoise_report"], report) and int(o["status"].item()) == 0
    figures = {}
    for k in ("Hs", "He", "eq", "Hest"):
        figures[k] = float(np.abs(o[k].cpu().numpy().reshape(ref[k].shape) - ref[k]).max() / np.abs(ref[k]).max())
    figures["slope"] = float(np.abs(o["slope"].cpu().numpy() - ref["slope"]).max())
    print(f"C3 {storage}: largest differences from the oracle {figures}")
    assert figures["Hs"] <= 1e-11 and figures["He"] <= 1e-11 and figures["slope"] <= 1e-11
    assert figures["eq"] <= 1e-12 and figures["Hest"] <= 1e-12
    bits = eng.unpack_bits(o["bits"]).cpu().numpy()
    sure = off_ties(ref["eq"])
    assert sure.mean() > 0.999 and np.array_equal(bits[sure], ref["bits"][sure])
    lean = eng.demod_frames(xt, starts, denoise=9.0)
    assert torch.equal(lean["bits"], o["bits"]) and torch.equal(lean["denoise_report"], report)


# ---- the two-phase form without the denoiser: what it gave before the feature ----------------------------------------
def test_split_path_without_denoise_is_what_it_was():
    """SHA-256 of every output of demod_frames(split=True) on the g1 loop-back fixture, recorded from the commit before the
    denoiser (tests/golden/denoise_nodrift.json)."""
    want = json.load(open(os.path.join(GOLD, "denoise_nodrift.json")))
    g = load("g1_n1024_qpsk")
    eng = engine_for(params_of(g))
    x = torch.from_numpy(g["r"]).cuda()
    starts = torch.from_numpy(np.asarray(g["peaks"][:-1]) + 2).cuda()
    o = eng.demod_frames(x, starts, want=("eq", "Hs", "He", "slope", "Hest"), split=True)
    got = {k: hashlib.sha256(o[k].cpu().numpy().tobytes()).hexdigest() for k in ("bits", "eq", "Hs", "He", "slope", "Hest")}
    assert got == want


# ---- the façade ----------------------------------------------------------------------------------------------------
# The façade fits the phase slope over carriers [500, 1000) as the reference does (OFDM.py:462), which mode A2's band holds
# and the N = 1024 geometry does not: its round trip runs at mode A2 (N = 4096, CP = 224, carriers 100 .. 1499) with
# no_pilots = 2, packet_length = 12, two packets; channel, noise and conditions as at the small geometry.
def a2_short():
    return dataclasses.replace(modeA2_params(load("g6_realrec")["known_bits"]), P=2, D=12)


def facade_stream(coded, seed, F):
    """tests/denoise_ref.py::noisy_stream carrying `coded`: -> r"""
    p = a2_short()
    rng = np.random.default_rng(seed)
    fill = p.const_points[rng.integers(0, 4, size=p.K - p.C)]
    clean = orc.tx_stream(coded, fill, p, lead=300, tail=400)
    r = np.convolve(clean, DR.sparse_channel(rng, 24, 5.0))[: len(clean)]
    starts = 300 + np.arange(F) * p.frame_len + p.Lc
    body = np.concatenate([r[s: s + p.M * p.S] for s in starts])
    noise = [np.random.default_rng(seed + 1 + b).standard_normal(len(r)) * np.sqrt(np.mean(body ** 2) / 10.0 ** 0.6) for b in range(2)]
    return r + noise[0], r + noise[1]


@pytest.mark.parametrize("encoding", ["None", "QCLDPC-1/2"])
def test_facade_round_trip(encoding):
    from gf3_audio_modem_amd.OFDM import receiver
    F = 2
    p = a2_short()
    rx = receiver("A2", encoding=encoding, no_pilots=2, packet_length=12)
    rx.llr_weighting = "noise" if encoding != "None" else "csi"
    rng = np.random.default_rng(31)
    per_packet = rx.packet_length * rx.data_bits_per_symbol
    if encoding == "None":
        payload = rng.integers(0, 2, size=F * per_packet)
        coded = payload
    else:
        payload = rng.integers(0, 2, size=768 * (F * per_packet // 1536))
        coded = np.asarray(rx.encode(payload))
        coded = np.concatenate([coded, rng.integers(0, 2, size=F * per_packet - len(coded))])
    r, r_b = facade_stream(coded.astype(np.uint8), seed=32, F=F)
    eng = rx._engine(np.dtype("float64"))
    starts = (eng.sync_stream(eng._samples(r)) + 2)[:-1].cpu().numpy()
    assert len(starts) == F
    plain = rx.receive(r)[0]
    assert rx.last_denoise_report is None
    r2, rep = DR.emulate(r, starts, p)                               # the CPU's prediction of the denoised path
    rx.channel_denoising = True
    got, Hs0, He0 = rx.receive(r)
    report = rx.last_denoise_report
    assert report.shape == (F, 2, 5) and report.dtype == np.float64 and (report[:, :, 4] == 1).all()
    np.testing.assert_array_equal(report[:, :, 1:], rep[:, :, 1:])
    ref = orc.demod_frames(r2, starts, p)
    assert np.abs(Hs0 - ref["Hs"][0]).max() <= 1e-11 * np.abs(ref["Hs"][0]).max()      # the returned estimate is the denoised one
    assert np.abs(He0 - ref["He"][0]).max() <= 1e-11 * np.abs(ref["He"][0]).max()
    if encoding == "None":
        sure = off_ties(ref["eq"])
        assert sure.mean() > 0.999 and np.array_equal(got[sure], ref["bits"][sure])
    else:                                                            # the coded chain itself, fed the emulated stream
        rx.channel_denoising = False
        predicted = rx.receive(r2)[0]
        rx.channel_denoising = True
        assert np.array_equal(got, predicted)
    n = len(payload)
    e_plain, e_dn = int(np.sum(plain[:n] != payload)), int(np.sum(got[:n] != payload))
    print(f"{encoding}: bit errors {e_plain} plain, {e_dn} denoised of {n}: ratio {e_dn / max(e_plain, 1):.3f}")
    assert e_dn < 0.8 * e_plain
    if encoding == "None":
        rx.receive_diversity([r, r_b])
        assert rx.last_denoise_report.shape == (2, F, 2, 5) and (rx.last_denoise_report[:, :, :, 4] == 1).all()
        np.testing.assert_array_equal(rx.last_denoise_report[0], report)
        rx.channel_denoising = False
        rx.receive_diversity([r, r_b])
        assert rx.last_denoise_report is None


# ---- the real recording ----------------------------------------------------------------------------------------------
def test_real_recording():
    """g6: three packets of the reference's geometry recorded in a room, 8-bit samples.  The denoiser runs; each row either
    applies with at most N/4 taps or passes through.  The figures are printed (DESIGN §12 holds them); no bound on them."""
    g = load("g6_realrec")
    p = modeA2_params(g["known_bits"])
    eng = engine_for(p, in_dtype=torch.uint8)
    starts = np.asarray(g["peaks"][:-1]) + 2
    psum, report = eng.denoise_pilots(torch.from_numpy(g["wav_u8"]).cuda(), starts)
    rep = report.cpu().numpy()
    print("g6 (v, kept, post, pre, applied) per packet and side:", np.round(rep, 3).tolist())
    assert rep.shape == (len(starts), 2, 5) and np.isfinite(rep).all() and np.isfinite(psum.cpu().numpy()).all()
    for row in rep.reshape(-1, 5):
        assert row[4] in (0.0, 1.0) and (row[4] == 0.0 or row[1] <= p.N // 4)
