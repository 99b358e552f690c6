"""Transmit diversity on the GPU: gf3_stbc_slope and gf3_stbc_detect against the NumPy restatement (tests/stbc_ref.py), edge
inputs and argument checks, and transmit_stbc -> the scenario's room -> receive_stbc end to end from ONE microphone
(tests/test_stbc_cpu.py holds the CPU form and settles the coded level).  The guard-band rows of the two entries are in
tests/test_bounds_stbc_gpu.py.  Helpers and shapes are those of tests/test_mimo_gpu.py: N = 1024, data bins 5 .. 399
(C = 395: two 256-carrier tiles, the second partial), fit range [10, 300), F = 3."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import mimo_ref as MR
from tests import stbc_ref as SR
from tests import tables as T
from tests.joint_checks import held_to_the_restatement
from tests.test_mimo_gpu import LEAD, TAIL, detect_inputs, engine_of, facade, oracle_params, quiet, resampled, same_bytes, small_params
from tests.test_stbc_cpu import LEVEL_DB, MIC

pytestmark = pytest.mark.gpu
F3 = 3
SLOPE_ATOL = 1e-11                                          # what tests/test_gpu_parity.py holds the demodulator's slope to


# ---- gf3_stbc_slope ----------------------------------------------------------------------------------------------------
def slope_inputs(p, F, B, seed, null=False):
    """B estimate sets [F, 2, 2, K]: the end block is the start block turned by 3.1 + 2e-4 k rad (the planted slope; the
    offset puts the angles at the +-pi seam, so the unwrap has work) and jittered by 0.1 rad and 10 % per carrier.  null:
    path (branch 0, column 0) scaled by 1e-6 over carriers 100 .. 119, inside the fit range, in both blocks."""
    rng = np.random.default_rng(seed)
    k = np.arange(p.K)
    Hs = []
    for _ in range(B):
        H = np.zeros((F, 2, 2, p.K), dtype=complex)
        H[:, 0] = (rng.normal(size=(F, 2, p.K)) + 1j * rng.normal(size=(F, 2, p.K))) * 0.7
        H[:, 1] = H[:, 0] * (1 + 0.1 * rng.normal(size=(F, 2, p.K))) * np.exp(1j * (3.1 + 2e-4 * k + 0.1 * rng.normal(size=(F, 2, p.K))))
        Hs.append(H)
    if null:
        Hs[0][:, :, 0, 100:120] *= 1e-6
    return Hs


@pytest.mark.parametrize("B", [1, 2, 4])
def test_slope_against_the_restatement(B):
    p = small_params(P=2, D=6)
    eng = engine_of(p)
    for null in (False, True):
        Hs = slope_inputs(p, F3, B, 40 + B, null)
        ref = SR.joint_slope(Hs, p)
        slope = eng.stbc_slope(Hs)
        got = slope.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (F3,)
        print(f"B {B}, null {null}: slope {got}, worst deviation from the restatement {np.abs(got - ref).max():.2e}")
        np.testing.assert_allclose(got, ref, rtol=0, atol=SLOPE_ATOL)
        assert np.abs(got - 2e-4).max() < 2e-4              # (the planted slope is what comes out, jitter apart)
        assert same_bytes(slope, eng.stbc_slope(Hs))
    # a NaN estimate inside the fit range: that packet's slope alone; outside the fit range: none
    Hs = [h.copy() for h in Hs]
    Hs[B - 1][1, 1, 1, 150] = complex(np.nan, 0.0)
    Hs[0][2, 0, 0, 400] = complex(0.0, np.inf)
    got = eng.stbc_slope(Hs).cpu().numpy()
    assert np.isnan(got[1]) and np.array_equal(got[[0, 2]], slope.cpu().numpy()[[0, 2]])
    assert np.array_equal(np.isnan(SR.joint_slope(Hs, p)), [False, True, False])


# ---- gf3_stbc_detect ---------------------------------------------------------------------------------------------------
def check_detect(p, eng, Ys, Hs, slope, packets=None):
    """One call against the restatement (on `packets` alone where given), the signs against its joint argmin, a second
    call's bytes -> the LLRs.  The comparison is check_detect's of tests/test_mimo_gpu.py."""
    llr = eng.stbc_detect(Ys, Hs, slope)
    got = llr.cpu().numpy()
    F = np.asarray(Hs[0]).shape[0]
    assert got.dtype == np.float32 and got.shape == (F, p.D, p.C, 2)
    assert same_bytes(llr, eng.stbc_detect(Ys, Hs, slope))
    part = got
    if packets is not None:
        rows = (np.asarray(packets)[:, None] * p.D + np.arange(p.D)).reshape(-1)
        Ys, Hs, slope = [y[rows] for y in Ys], [h[packets] for h in Hs], slope[packets]
        part = got[packets]
    ref, pair = SR.detect(Ys, Hs, slope, p)
    held_to_the_restatement(part, ref, pair, p.const_bits)
    return got


@pytest.mark.parametrize("kind,P,D", [("qpsk", 2, 2), ("qpsk", 4, 6), ("shuffled", 2, 14), ("qpsk_rot", 4, 6)])
def test_detect_against_the_restatement(kind, P, D):
    """B = 1 .. 4 with the reference's QPSK, a 4-point table that is no grid, and on a scattered carrier map; a slope of a
    few 1e-3 rad per carrier, so the two slots of a pair differ and G01 is not zero."""
    p = small_params(P=P, D=D, table=T.TABLES["qpsk_rot"] if kind == "qpsk_rot" else None,
                     carriers=T.MAPS["shuffled"](511) if kind == "shuffled" else None)
    eng = engine_of(p)
    Ys, Hs, slopes = detect_inputs(p, F3, 4, len(kind) + P + D)
    G00, _, G01 = SR.sufficient(Ys[:1], Hs[:1], slopes[0], p)[:3]
    assert np.abs(G01).mean() > 1e-4 * G00.mean()
    for B in (1, 2, 3, 4):
        check_detect(p, eng, Ys[:B], Hs[:B], slopes[0])


def test_detect_runs_of_pairs_per_workgroup():
    """64 packets of 100 symbols on 257 carriers: a workgroup then takes a run of consecutive PAIRS (4 of the 50 on 256
    compute units, the last run 2) and advances its phasors from symbol to symbol; three packets are held to the
    restatement."""
    p = small_params(P=2, D=100, carriers=np.arange(5, 262))
    eng = engine_of(p)
    Ys, Hs, slopes = detect_inputs(p, 64, 2, 61)
    check_detect(p, eng, Ys, Hs, slopes[0], packets=[0, 37, 63])


@pytest.mark.parametrize("N", [2048, 4096, 8192])
def test_detect_at_the_other_transform_sizes(N):
    p = small_params(P=2, D=2, N=N)
    eng = engine_of(p)
    Ys, Hs, slopes = detect_inputs(p, 2, 2, N)
    check_detect(p, eng, Ys, Hs, slopes[0])
    ref = SR.joint_slope(Hs, p)
    np.testing.assert_allclose(eng.stbc_slope(Hs).cpu().numpy(), ref, rtol=0, atol=SLOPE_ATOL)


def test_detect_edge_inputs():
    p = small_params(P=2, D=6)
    eng = engine_of(p)
    Ys, Hs, slopes = detect_inputs(p, F3, 2, 21)
    Ys, Hs, slope = [y.copy() for y in Ys], [h.copy() for h in Hs], slopes[0]
    bins = p.data_carriers
    cell = lambda f, l: f * p.D + l
    Ys[0][cell(0, 3), bins[17]] = complex(np.nan, 0.0)     # y at slot 2j + 1 of one branch: the other decides the PAIR alone
    Ys[1][cell(1, 4), bins[300]] = complex(1.0, np.inf)    # y at slot 2j
    Hs[0][2, 1, 1, bins[40] - 1] = complex(0.0, np.nan)    # one estimate of one branch: that carrier of that packet, every pair
    for y in Ys:                                           # every branch, one slot: nothing is left of the pair
        y[cell(1, 1), bins[258]] = complex(np.nan, np.nan)
    got = check_detect(p, eng, Ys, Hs, slope)
    assert np.isfinite(got).all()
    alone = [eng.stbc_detect([Ys[b]], [Hs[b]], slope).cpu().numpy() for b in range(2)]
    tol = dict(rtol=1e-6, atol=1e-9 * np.abs(got).max())
    np.testing.assert_allclose(got[0, 2:4, 17], alone[1][0, 2:4, 17], **tol)          # both symbols of the pair
    np.testing.assert_allclose(got[1, 4:6, 300], alone[0][1, 4:6, 300], **tol)
    np.testing.assert_allclose(got[2, :, 40], alone[1][2, :, 40], **tol)
    for b, (f, l, c) in ((0, (0, 2, 17)), (1, (1, 4, 300))):                          # ... and no other: the neighbours hold both branches
        assert not np.allclose(got[f, l, c + 1], alone[1 - b][f, l, c + 1], **tol)
        assert not np.allclose(got[f, (l + 2) % p.D, c], alone[1 - b][f, (l + 2) % p.D, c], **tol)
    dead = got[1, 0:2, 258]
    assert dead.shape == (2, 2) and not dead.any() and not np.signbit(dead).any()
    # B = 1: the branch's own NaN at slot 2j + 1 leaves +0 in both symbols of the pair, never -0, and the pairs around it whole
    one = alone[0]
    assert not one[0, 2:4, 17].any() and not np.signbit(one[0, 2:4, 17]).any() and one[0, 0:2, 17].all() and one[0, 4:6, 17].all()
    # a slope that is not finite: every branch is dead everywhere
    for bad in (np.inf, -np.inf, np.nan):
        sl = slope.copy()
        sl[1] = bad
        out = eng.stbc_detect(Ys, Hs, sl).cpu().numpy()
        assert not out[1].any() and not np.signbit(out[1]).any() and np.array_equal(out[[0, 2]], got[[0, 2]])
    out = eng.stbc_detect(Ys, Hs, np.full(F3, np.inf)).cpu().numpy()
    assert not out.any() and not np.signbit(out).any()


def test_argument_checks():
    from gf3_audio_modem_amd import _lib
    p = small_params(P=2, D=6)
    eng = engine_of(p)
    F = 2
    Ys, Hs, slopes = detect_inputs(p, F, 2, 8)
    slope = slopes[0]
    n = F * p.D * p.C * 2
    bad = [dict(Ys=[]), dict(Ys=Ys * 3, Hs=Hs * 3), dict(Hs=Hs[:1]), dict(Ys=[Ys[0], Ys[1][: p.D]]), dict(Ys=[y[:-1] for y in Ys]),
           dict(Hs=[Hs[0], Hs[1][:1]]), dict(slope=slope[:1]), dict(slope=np.stack([slope, slope])),
           dict(out=torch.empty(n - 1, dtype=torch.float32, device="cuda")), dict(out=torch.empty(n, dtype=torch.float64, device="cuda")),
           dict(out=torch.empty(2 * n, dtype=torch.float32, device="cuda")[::2])]
    for kw in bad:
        with pytest.raises(ValueError, match="stbc_detect"):
            eng.stbc_detect(**{**dict(Ys=Ys, Hs=Hs, slope=slope), **kw})
    for Hb in ([], Hs * 3, [Hs[0], Hs[1][:1]], [Hs[0].reshape(-1)[:-1]]):
        with pytest.raises(ValueError, match="stbc_slope"):
            eng.stbc_slope(Hb)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    o = eng.stbc_detect(Ys, Hs, slope, out=out)
    assert o.data_ptr() == out.data_ptr() and same_bytes(o, eng.stbc_detect(Ys, Hs, slope))
    again = eng.stbc_detect(Ys[:1], Hs[:1], slope, out=out)                            # `out` reused by another call
    assert again.data_ptr() == out.data_ptr() and same_bytes(again, eng.stbc_detect(Ys[:1], Hs[:1], slope))
    empty = eng.stbc_detect([np.zeros((0, 513), complex)] * 2, [np.zeros((0, 2, 2, 511), complex)] * 2, np.zeros(0))
    assert empty.shape == (0, p.D, p.C, 2) and eng.stbc_slope([np.zeros((0, 2, 2, 511), complex)]).shape == (0,)
    # contexts the pair refuses: an odd D, an odd P, a 16-point table -- the façade and the library both
    odd_d, odd_p, p16 = small_params(P=2, D=7), small_params(P=3, D=6), small_params(P=2, D=6, table=orc.square_qam_table(4))
    e_d, e_p, e16 = engine_of(odd_d), engine_of(odd_p), engine_of(p16)
    Y7 = [np.zeros((F * 7, 513), complex)] * 2
    with pytest.raises(ValueError, match="stbc_detect.*even D"):
        e_d.stbc_detect(Y7, Hs, slope)
    with pytest.raises(ValueError, match="stbc_slope.*even D"):
        e_d.stbc_slope(Hs)
    with pytest.raises(ValueError, match="stbc_detect.*even number of pilot symbols"):
        e_p.stbc_detect(Ys, Hs, slope)
    with pytest.raises(ValueError, match="stbc_slope.*even number of pilot symbols"):
        e_p.stbc_slope(Hs)
    with pytest.raises(ValueError, match="stbc_detect.*mu = 2"):
        e16.stbc_detect(Ys, Hs, slope)
    # the raw ABI
    lib = eng.lib
    dY, dH = [eng._dev(y) for y in Ys], [eng._dev(h) for h in Hs]
    dS, dO = eng._dev(slope, torch.float64), torch.empty(F, dtype=torch.float64, device="cuda")
    tab = lambda xs: (C.c_void_p * len(xs))(*[None if x is None else x.data_ptr() for x in xs])
    Yt, Ht, St, q, so = tab(dY), tab(dH), _lib.ptr(dS), _lib.ptr(out), _lib.ptr(dO)
    det = lambda *a: lib.gf3_stbc_detect(*a, None)
    assert det(eng._h, 2, Yt, Ht, St, 0, q) == 0 and det(eng._h, 9, None, None, None, 0, None) == 0      # F == 0: a no-op
    cases = {"no context": (None, 2, Yt, Ht, St, F, q), "B = 0": (eng._h, 0, Yt, Ht, St, F, q), "B = 5": (eng._h, 5, Yt, Ht, St, F, q),
             "no spectra": (eng._h, 2, None, Ht, St, F, q), "no estimates": (eng._h, 2, Yt, None, St, F, q),
             "no slope": (eng._h, 2, Yt, Ht, None, F, q), "null spectrum": (eng._h, 2, tab([dY[0], None]), Ht, St, F, q),
             "null estimate": (eng._h, 2, Yt, tab([None, dH[1]]), St, F, q), "no output": (eng._h, 2, Yt, Ht, St, F, None),
             "F < 0": (eng._h, 2, Yt, Ht, St, -1, q), "too many packets": (eng._h, 2, Yt, Ht, St, 65536, q),
             "16-QAM": (e16._h, 2, Yt, Ht, St, F, q), "odd D": (e_d._h, 2, Yt, Ht, St, F, q), "odd P": (e_p._h, 2, Yt, Ht, St, F, q),
             "odd D, F = 0": (e_d._h, 2, Yt, Ht, St, 0, q)}
    for text, args in cases.items():
        assert det(*args) == _lib.GF3_EINVAL, text
        assert b"gf3_stbc_detect" in lib.gf3_last_error(None), text
    slo = lambda *a: lib.gf3_stbc_slope(*a, None)
    assert slo(eng._h, 2, Ht, 0, so) == 0 and slo(eng._h, 9, None, 0, None) == 0
    cases = {"no context": (None, 2, Ht, F, so), "B = 0": (eng._h, 0, Ht, F, so), "B = 5": (eng._h, 5, Ht, F, so),
             "no estimates": (eng._h, 2, None, F, so), "null estimate": (eng._h, 2, tab([None, dH[1]]), F, so),
             "no output": (eng._h, 2, Ht, F, None), "F < 0": (eng._h, 2, Ht, -1, so), "too many packets": (eng._h, 2, Ht, 1 << 30, so),
             "odd D": (e_d._h, 2, Ht, F, so), "odd P": (e_p._h, 2, Ht, F, so)}
    for text, args in cases.items():
        assert slo(*args) == _lib.GF3_EINVAL, text
        assert b"gf3_stbc_slope" in lib.gf3_last_error(None), text
    torch.cuda.synchronize()


# ---- end to end --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recordings(encoding):
    """Two packets through transmit_stbc and the scenario's room, noiseless -> (payload, stereo signal, [mic 0, mic 1])"""
    rx = facade(encoding)
    n = 9 * 768 if encoding.startswith("QCLDPC") else 2 * 4 * 1800
    payload = np.random.default_rng(3).integers(0, 2, size=n)
    np.random.seed(5)                                       # (the fill of the last packet, the filler of the unused carriers)
    tx2 = quiet(rx.transmit_stbc, payload)
    assert tx2.dtype == np.float64 and tx2.shape == (2, 3 * rx.chirp_length + 2 * 12 * 4320) and rx.no_packets == 2
    tx2 = np.concatenate([np.zeros((2, LEAD)), tx2, np.zeros((2, TAIL))], axis=1)
    return payload, tx2, MR.through(tx2)


def test_transmit_stbc_format():
    """The restatement builds the same two streams from the same bits and filler; row 0's pilots, chirps and even slots are
    transmit()'s own samples."""
    payload, tx2, _ = recordings("None")
    rx = facade("None")
    p = oracle_params(rx)
    np.random.seed(5)
    np.random.binomial(n=1, p=0.5, size=(0,))
    fill = rx.random_qpsk()
    ref = SR.tx_stbc(payload, fill, p, lead=LEAD, tail=TAIL)
    assert tx2.shape == ref.shape and np.abs(tx2 - ref).max() <= 1e-12 * np.abs(ref).max()
    np.random.seed(5)
    plain = quiet(rx.transmit, payload)
    Lc, S = rx.chirp_length, 4320
    assert len(plain) == tx2.shape[1] - LEAD - TAIL
    for f in range(2):
        at = LEAD + f * (Lc + 12 * S)
        mine, theirs = tx2[0, at: at + Lc + 12 * S], plain[at - LEAD: at - LEAD + Lc + 12 * S]
        assert np.array_equal(mine[:Lc + 4 * S], theirs[:Lc + 4 * S]) and np.array_equal(mine[Lc + 8 * S:], theirs[Lc + 8 * S:])
        assert np.array_equal(mine[Lc + 4 * S: Lc + 5 * S], theirs[Lc + 4 * S: Lc + 5 * S])
        assert np.array_equal(mine[Lc + 6 * S: Lc + 7 * S], theirs[Lc + 6 * S: Lc + 7 * S])
        assert not tx2[1, at: at + Lc].any()
    assert rx.last_tx_report is not None


@pytest.mark.parametrize("encoding", ["None", "XOR", "QCLDPC-1/2"])
def test_receive_stbc_noiseless_is_exact(encoding):
    payload, tx2, rec = recordings(encoding)
    rx = facade(encoding)
    p = oracle_params(rx)
    for signals in ([rec[0]], [rec[1]], rec, np.stack(rec)):
        bits, Hs0, He0 = quiet(rx.receive_stbc, signals)
        assert bits.dtype == np.int64 and np.array_equal(bits[: len(payload)], payload) and rx.no_packets == 2
        # what it publishes, against the restatement on the same samples
        o = SR.receive_stbc(list(signals), p)
        assert rx.last_branch_starts.dtype == np.int64 and np.array_equal(rx.last_branch_starts, o["starts"])
        sl = rx.last_stbc_slope
        assert sl.dtype == np.float64 and sl.shape == (2,)
        print(f"{encoding}, {len(signals)} recording(s): slope {sl}, restatement {o['slope']}")
        # (the estimates agree to 1e-12 relative; over the fit range's dynamic of <= 1e4 that is <= 1e-8 rad in a carrier's
        #  angle, times the fit's lever 3 / L per carrier)
        np.testing.assert_allclose(sl, o["slope"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(Hs0, o["H"][0][0, 0, 0], rtol=1e-9, atol=1e-9 * np.abs(Hs0).max())
        np.testing.assert_allclose(He0, o["H"][0][0, 1, 0], rtol=1e-9, atol=1e-9 * np.abs(He0).max())
        assert rx.last_clock_ppm is None and rx.sync_report is None
        if encoding.startswith("QCLDPC"):
            assert rx.last_decode_report["codewords"] == 9 and rx.last_decode_report["inner_failed"] == 0
    if encoding == "None":
        with pytest.raises(ValueError, match=r"receive_stbc: the recordings hold different numbers of packets: \[2, 5\]"):
            quiet(rx.receive_stbc, [rec[0], np.concatenate([rec[1], rec[1]])])


def test_receive_stbc_coded_at_the_settled_level_from_one_microphone():
    """Microphone 1 alone at LEVEL_DB: every codeword decodes and the payload is exact.  The same samples received as
    "None" give the signs of the raw LLRs; they are the restatement's except where its LLR is unclear: below 1e-6 of the
    largest (both chains' LLRs are float32, and their inputs -- estimates, spectra, slope -- agree to 1e-8 rad or better)."""
    payload, tx2, rec = recordings("QCLDPC-1/2")
    rx = facade("QCLDPC-1/2")
    noisy = SR.add_noise([rec[MIC]], SR.body_rms(tx2), LEVEL_DB, [MIC])
    bits, _, _ = quiet(rx.receive_stbc, noisy)
    print(f"{LEVEL_DB} dB, microphone {MIC}: report {rx.last_decode_report}, slope {rx.last_stbc_slope}")
    assert rx.last_decode_report["codewords"] == 9 and rx.last_decode_report["inner_failed"] == 0
    assert np.array_equal(bits[: len(payload)], payload)
    raw, _, _ = quiet(facade("None").receive_stbc, noisy)
    o = SR.receive_stbc(noisy, oracle_params(rx))
    unclear = np.abs(o["llr"]) <= 1e-6 * np.abs(o["llr"]).max()
    differ = raw != o["bits"]
    print(f"raw signs that differ from the restatement's: {int(differ.sum())} of {len(raw)}; unclear cells {int(unclear.sum())}")
    assert raw.shape == o["bits"].shape and not (differ & ~unclear).any()


def test_receive_stbc_with_outer_code_and_crc():
    rx = facade("QCLDPC-1/2", outer_code=(2, 1), codeword_crc=True)
    payload = np.random.default_rng(4).integers(0, 2, size=1000)
    np.random.seed(6)
    tx2 = quiet(rx.transmit_stbc, payload)
    rec = MR.through(np.concatenate([np.zeros((2, LEAD)), tx2, np.zeros((2, TAIL))], axis=1))
    bits, _, _ = quiet(rx.receive_stbc, [rec[0]])
    report = rx.last_decode_report
    assert rx.no_packets == tx2.shape[1] // (rx.chirp_length + 12 * 4320)
    assert report["inner_failed"] == 0 and report["groups_failed"] == 0 and report["crc_failed"] == 0
    assert np.array_equal(bits[:1000], payload) and not bits[1000:].any()


def test_stbc_at_the_sound_cards_own_rate():
    """output_rate on the transmitter converts both rows, input_rate on the receiver the recording: 44.1 kHz on both ends"""
    payload, _, _ = recordings("None")
    rx = facade("None", output_rate=44100.0, input_rate=44100.0)
    np.random.seed(5)
    tx2 = quiet(rx.transmit_stbc, payload)
    n48 = 3 * rx.chirp_length + 24 * 4320
    assert tx2.shape[0] == 2 and abs(tx2.shape[1] - n48 * 44100 / 48000) < 2 and rx.last_tx_report["output_samples"] == tx2.shape[1]
    rec = MR.through(np.concatenate([np.zeros((2, LEAD)), tx2, np.zeros((2, TAIL))], axis=1))
    bits, _, _ = quiet(rx.receive_stbc, [rec[1]])
    assert np.array_equal(bits, payload)
    assert np.array_equal(rx.last_input_rate, [44100.0])


def test_receive_stbc_local_sync_rule():
    payload, tx2, rec = recordings("None")
    rx = facade("None", sync_rule="local")
    bits, _, _ = quiet(rx.receive_stbc, [rec[0]])
    assert np.array_equal(bits, payload)
    rho = np.asarray(rx.sync_report["rho"])
    assert rho.shape == (1, 3) and (rho > 0.3).all() and rx.sync_report["threshold"] == 0.3


def test_receive_stbc_under_clock_correction():
    """The recording of tests/test_mimo_gpu.py's clock test: taken by a sound card 30 ppm fast; clock_correction = 30.0"""
    payload, tx2, rec = recordings("None")
    rx = facade("None", clock_correction=30.0)
    bits, _, _ = quiet(rx.receive_stbc, [resampled(rec[0], 30e-6)])
    assert np.array_equal(bits, payload)
    assert rx.last_clock_ppm.shape == (1,) and (rx.last_clock_ppm == 30.0).all() and rx.last_clock_ppm_packets is None
