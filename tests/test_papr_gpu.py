"""Tone reservation on the GPU: papr_kernel against its NumPy restatement (tests/papr_ref.py), the receiver's view of rows
sent with tones, the parts of a row the tones must not touch, the peak report, determinism, the degenerate cases and the
façade end to end.

Tolerances.  Tones: atol = I x 1e-12 x L -- the 1e-12 that test_tx_frames_matches_reference_stream grants one transform,
once per iteration (the map from one iterate to the next is continuous in its input).  Peaks and rms: a symbol is one more
transform away from its tones, and a deviation d on one tone moves a sample by at most 2 d / N, so
(I + 1) x 1e-12 x peak + 2 Ku / N x the tones' atol.  The best index is compared as an integer: the restatement's two
smallest iterate peaks must not lie within 1e-9 (relative) of each other on more than 1 % of the symbols; the seeds below
leave none.  Measured on the MI355X: tones 8.5e-16 .. 2.6e-14, peaks and rms within 3e-4 of their bound; on
the cases of MORE_GEOMETRIES (N = 2048 and 8192, labels of 1, 3, 5, 7 and 8 bits; the same bounds, N = 8192 inside the
1e-12 that test_rfft_batch grants a transform up to that size): tones 7.7e-16 .. 6.6e-15, peaks and rms within 5e-5 of their
bound."""
import contextlib
import io

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import papr_ref as PR
from tests.test_papr_cpu import MORE_GEOMETRIES, more_params, payload_bits, scattered, small_params
from tests.util import engine_for, load, modeA2_params

pytestmark = pytest.mark.gpu
CASES = {}
F_SMALL = 3


def _params(name):
    if name in MORE_GEOMETRIES:
        return more_params(name)
    if name == "contig":
        return small_params(), F_SMALL
    if name == "scattered":
        return small_params(carriers=scattered()), F_SMALL
    if name == "one_tone":                                               # Ku = 1: every carrier but bin 200 carries data
        return small_params(carriers=np.delete(np.arange(1, 512), 199)), F_SMALL
    import dataclasses
    a2 = dataclasses.replace(modeA2_params(load("g6_realrec")["known_bits"]), P=1, D=4)
    if name == "c3_qpsk":                                                # the standard's longest prefix and narrowest band: S = 5280,
        return dataclasses.replace(a2, CP=1184, hi=1000, P=2, D=2), 2    # Ku = 1147 reserved tones against C = 900 data carriers
    if name == "a2_qpsk":
        return a2, 2
    pts, bt = orc.square_qam_table(4)
    known = np.tile(a2.known_bits, 2)[: a2.K * 4]
    return dataclasses.replace(a2, const_points=pts, const_bits=bt, known_bits=known), 2


def case(name, iterations=16):
    """Parameters, payload, restatement and engine of one case: computed once, shared, left unchanged."""
    key = (name, iterations)
    if key not in CASES:
        p, F = _params(name)
        bits = payload_bits(name, p, F)
        ref = PR.tone_reserve(bits, p, 6.0, 6.0, iterations)
        eng = CASES[(name, 16)][4] if (name, 16) in CASES else engine_for(p, max_window=256)
        CASES[key] = (p, F, orc.pack_bits(bits, p.D * p.C * p.mu), ref, eng)
    return CASES[key]


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# (MORE_GEOMETRIES: papr_kernel<1024> at N = 2048, papr_kernel<4096> at N = 8192, labels of 1, 3, 5, 7 and 8 bits)
NAMES = ["contig", "scattered", "one_tone", "a2_qpsk", "a2_qam16", "c3_qpsk"] + MORE_GEOMETRIES


# ---- 1. against the restatement, 4. the peak report, 5. determinism -----------------------------------------------------
@pytest.mark.parametrize("iterations", [16, 3])
@pytest.mark.parametrize("name", NAMES)
def test_kernel_against_the_restatement(name, iterations):
    p, F, packed, (want, wrep, peaks), eng = case(name, iterations)
    Ku, L = p.K - p.C, 10.0 ** (6.0 / 20.0)
    ties = np.array([PR.near_tie(q) for q in peaks]).reshape(F, p.D)
    assert ties.mean() <= 0.01                                           # (the condition on the seeds, by the restatement alone)
    tones, report = eng.tone_reserve(packed, 6.0, 6.0, iterations)
    assert tones.dtype == torch.complex128 and tuple(tones.shape) == (F, p.D, Ku) and tuple(report.shape) == (F, p.D, 4)
    got, rep = tones.cpu().numpy(), report.cpu().numpy()
    atol = iterations * 1e-12 * L
    ptol = (iterations + 1) * 1e-12 * wrep[..., 0] + 2.0 * Ku / p.N * atol
    figures = {"tones": float(np.abs(got - want)[~ties].max()), "peak0": float((np.abs(rep[..., 0] - wrep[..., 0]) / ptol).max()),
               "best peak": float((np.abs(rep[..., 1] - wrep[..., 1]) / ptol).max()),
               "rms": float((np.abs(rep[..., 3] - wrep[..., 3]) / ptol)[~ties].max())}
    print(f"{name} I={iterations}: largest |tone - restatement| {figures['tones']:.2e} (atol {atol:.1e}); peak0, best peak, rms in "
          f"units of their bound {figures['peak0']:.2e} {figures['best peak']:.2e} {figures['rms']:.2e}; best index mean "
          f"{rep[..., 2].mean():.1f}, peak {wrep[..., 0].mean():.4f} -> {wrep[..., 1].mean():.4f}")
    assert figures["tones"] <= atol
    assert np.array_equal(rep[..., 2][~ties], wrep[..., 2][~ties])
    assert figures["peak0"] <= 1.0 and figures["best peak"] <= 1.0 and figures["rms"] <= 1.0
    # the report: never worse than a zero filler, every tone within its limit
    assert (rep[..., 1] <= rep[..., 0]).all() and np.abs(got).max() <= L * (1 + 1e-12)
    # 2 x the reported peak is the largest sample of that symbol as gf3_tx_frames_ex sends it
    rows = eng.tx_frames(packed, np.zeros(p.K, complex), out_dtype=torch.float64, tones=tones).cpu().numpy()
    body = rows[:, p.Lc:].reshape(F, 2 * p.P + p.D, p.S)[:, p.P:p.P + p.D]
    sent_peak = np.abs(body).max(axis=2)
    assert np.abs(2.0 * rep[..., 1] - sent_peak).max() <= 1e-12 * sent_peak.max()
    zero = eng.tx_frames(packed, np.zeros(p.K, complex), out_dtype=torch.float64).cpu().numpy()
    zero_peak = np.abs(zero[:, p.Lc:].reshape(F, 2 * p.P + p.D, p.S)[:, p.P:p.P + p.D]).max(axis=2)
    assert np.abs(2.0 * rep[..., 0] - zero_peak).max() <= 1e-12 * zero_peak.max()
    again = eng.tone_reserve(packed, 6.0, 6.0, iterations)
    assert same_bytes(again[0].cpu().numpy(), got) and same_bytes(again[1].cpu().numpy(), rep)


# ---- 2. the receiver is unaffected, 3. the untouched parts -------------------------------------------------------------
@pytest.mark.parametrize("name", ["contig", "scattered", "a2_qam16", "c3_qpsk", "n2048_contig", "n2048_scattered", "n8192_contig"])
def test_receiver_unaffected_and_untouched_parts(name):
    p, F, packed, _, eng = case(name)
    rs = np.random.RandomState(len(name))
    filler = np.zeros(p.K, dtype=complex)
    filler[PR.reserved_bins(p) - 1] = rs.choice(np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) / np.sqrt(2), size=p.K - p.C)
    tones, _ = eng.tone_reserve(packed)
    gaps = rs.randint(0, 200, F)
    stride = p.frame_len + 256
    kw = dict(stride=stride, gaps=gaps, out_dtype=torch.float64)
    plain = eng.tx_frames(packed, filler, **kw)
    sent = eng.tx_frames(packed, filler, tones=tones, **kw)
    a, b = plain.cpu().numpy(), sent.cpu().numpy()
    # chirp, gaps, pilots and the zeros after the packet: the same bytes; every prefix is its symbol's tail
    M = 2 * p.P + p.D
    for f in range(F):
        g = int(gaps[f])
        assert same_bytes(a[f, :g + p.Lc], b[f, :g + p.Lc]) and same_bytes(a[f, g + p.frame_len:], b[f, g + p.frame_len:])
        assert not b[f, :g].any() and not b[f, g + p.frame_len:].any()
        sa, sb = (r[f, g + p.Lc: g + p.frame_len].reshape(M, p.S) for r in (a, b))
        pil = list(range(p.P)) + list(range(p.P + p.D, M))
        assert same_bytes(sa[pil], sb[pil]) and not same_bytes(sa[p.P:p.P + p.D], sb[p.P:p.P + p.D])
        assert same_bytes(sb[:, :p.CP], sb[:, p.S - p.CP:])
    # the default call is the _ex call with NULL tones and gain 1
    from gf3_audio_modem_amd import _lib
    out = torch.empty_like(plain)
    bits_d, fill_d, gaps_d = eng._dev(packed, torch.uint8), eng._dev(filler), eng._dev(gaps, torch.int64)
    assert eng.lib.gf3_tx_frames_ex(eng._h, _lib.ptr(bits_d), _lib.ptr(fill_d), _lib.ptr(gaps_d), F, _lib.ptr(out), stride,
                                    _lib.DT_F64, None, 1.0, None) == 0
    torch.cuda.synchronize()
    assert same_bytes(out.cpu().numpy(), a)
    # the data bins of every data symbol: what they were
    starts = np.arange(F) * stride + gaps + p.Lc
    off = (starts[:, None] + (p.P + np.arange(p.D))[None, :] * p.S + p.CP).reshape(-1)
    Xa, Xb = (eng.rfft_batch(r.reshape(-1), off).cpu().numpy()[:, p.data_carriers] for r in (plain, sent))
    assert np.abs(Xa - Xb).max() <= 1e-12 * np.abs(Xa).max()
    # sync + demodulation return the packed bits, also with the body raised to the chirp's level
    found = eng.sync_frames(sent, F, stride, -8, 248)
    assert np.array_equal(found.cpu().numpy(), starts)
    o = eng.demod_frames(sent, found, want=("Hs",))
    assert np.array_equal(o["bits"].cpu().numpy(), packed)
    body_peak = max(np.abs(b[f, int(gaps[f]) + p.Lc: int(gaps[f]) + p.frame_len]).max() for f in range(F))
    headroom_db = 20 * np.log10(np.abs(b[0, int(gaps[0]): int(gaps[0]) + p.Lc]).max() / body_peak)
    gain = 10.0 ** (headroom_db / 20.0)
    loud = eng.tx_frames(packed, filler, tones=tones, body_gain=gain, **kw)
    c = loud.cpu().numpy()
    for f in range(F):
        g = int(gaps[f])
        assert same_bytes(c[f, :g + p.Lc], b[f, :g + p.Lc])
        assert np.abs(c[f, g + p.Lc:] - gain * b[f, g + p.Lc:]).max() <= 1e-15 * gain * body_peak
    found2 = eng.sync_frames(loud, F, stride, -8, 248)
    assert np.array_equal(found2.cpu().numpy(), starts)
    o2 = eng.demod_frames(loud, found2, want=("Hs",))
    assert np.array_equal(o2["bits"].cpu().numpy(), packed)
    Hs, Hs2 = o["Hs"].cpu().numpy(), o2["Hs"].cpu().numpy()
    print(f"{name}: headroom {headroom_db:.2f} dB, |Hs(gain) - gain Hs| / max {np.abs(Hs2 - gain * Hs).max() / np.abs(gain * Hs).max():.1e}")
    assert np.abs(Hs2 - gain * Hs).max() <= 1e-12 * np.abs(gain * Hs).max()


# ---- 6. degenerate cases and refusals -------------------------------------------------------------------------------------
def test_degenerate_cases_and_refusals():
    from gf3_audio_modem_amd import _lib
    p, F, packed, _, eng = case("contig")
    Ku = p.K - p.C
    tones, report = eng.tone_reserve(packed, iterations=0)               # I = 0: zero tones, best = iterate 0
    rep = report.cpu().numpy()
    assert not tones.cpu().numpy().any() and (rep[..., 2] == 0).all() and same_bytes(rep[..., 0], rep[..., 1])
    tones, report = eng.tone_reserve(packed, target_db=13.0)             # nothing to clip: stops at iterate 0
    assert not tones.cpu().numpy().any() and (report.cpu().numpy()[..., 2] == 0).all()
    empty = eng.tone_reserve(np.zeros((0, eng.bytes_per_frame), np.uint8))
    assert tuple(empty[0].shape) == (0, p.D, Ku) and tuple(empty[1].shape) == (0, p.D, 4)
    lib, ptr = eng.lib, _lib.ptr
    bits_d = eng._dev(packed, torch.uint8)
    out = torch.full((F, p.D, Ku), 7.0, dtype=torch.complex128, device="cuda")
    rep_d = torch.full((F, p.D, 4), 7.0, dtype=torch.float64, device="cuda")
    assert lib.gf3_tone_reserve(eng._h, None, 0, 6.0, 6.0, 16, None, None, None) == 0          # F = 0
    for args in ((None, F, 6.0, 6.0, 16, ptr(out), ptr(rep_d)), (ptr(bits_d), F, 6.0, 6.0, 16, None, ptr(rep_d)),
                 (ptr(bits_d), F, 6.0, 6.0, 16, ptr(out), None), (ptr(bits_d), -1, 6.0, 6.0, 16, ptr(out), ptr(rep_d)),
                 (ptr(bits_d), F, float("nan"), 6.0, 16, ptr(out), ptr(rep_d)), (ptr(bits_d), F, 6.0, float("inf"), 16, ptr(out), ptr(rep_d)),
                 (ptr(bits_d), F, 6.0, 6.0, -1, ptr(out), ptr(rep_d)), (ptr(bits_d), F, 6.0, 6.0, 65, ptr(out), ptr(rep_d))):
        assert lib.gf3_tone_reserve(eng._h, *args, None) == _lib.GF3_EINVAL
        assert b"gf3_tone_reserve" in lib.gf3_last_error(None)
    rows = torch.full((F, p.frame_len), 7.0, dtype=torch.float64, device="cuda")
    for gain in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.gf3_tx_frames_ex(eng._h, ptr(bits_d), None, None, F, ptr(rows), p.frame_len, _lib.DT_F64, ptr(out), gain, None) == _lib.GF3_EINVAL
        assert b"body_gain" in lib.gf3_last_error(None)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (rep_d == 7.0).all() and (rows == 7.0).all()      # no refusal wrote anything
    with pytest.raises(ValueError, match="tones must be"):
        eng.tx_frames(packed, np.zeros(p.K, complex), tones=torch.zeros((F, p.D, Ku + 1), dtype=torch.complex128))
    full = engine_for(small_params(lo=1, hi=512), max_window=256)        # Ku = 0: no carrier is left
    bits0 = np.zeros((1, full.bytes_per_frame), np.uint8)
    with pytest.raises(ValueError, match="Ku = 0"):
        full.tone_reserve(bits0)
    assert lib.gf3_tx_frames_ex(full._h, ptr(bits_d), None, None, 1, ptr(rows), p.frame_len, _lib.DT_F64, ptr(out), 1.0, None) == _lib.GF3_EINVAL
    full.close()


# ---- 7. the façade, end to end ---------------------------------------------------------------------------------------------
def test_facade_end_to_end():
    from gf3_audio_modem_amd.OFDM import receiver
    message = np.random.default_rng(5).integers(0, 2, size=768 * 20)

    def run(option):
        tx = receiver("A2", encoding="QCLDPC-1/2", no_pilots=2, packet_length=8)
        tx.papr_reduction = option
        np.random.seed(23)
        with contextlib.redirect_stdout(io.StringIO()):
            sig = tx.transmit(message)
        return tx, sig

    tx, sig = run(True)
    ref, plain = run(False)
    assert tx.no_packets == 2 and len(sig) == len(plain)
    rep, rep0 = tx.last_tx_report, ref.last_tx_report
    print("with tones:", rep)
    print("reference filler:", rep0)
    assert set(rep) == set(rep0) | {"data_peak_zero_filler", "best_index_mean"}
    assert rep["data_peak"] <= rep["data_peak_zero_filler"]
    assert rep["chirp_peak"] == rep0["chirp_peak"] and rep["pilot_peak"] == rep0["pilot_peak"]
    S, Lc, P, D = tx.ofdm_symbol_size + tx.cp_length, tx.chirp_length, 2, 8
    a, b = (s[:-Lc].reshape(2, Lc + (2 * P + D) * S) for s in (sig, plain))
    assert same_bytes(sig[-Lc:], plain[-Lc:]) and same_bytes(a[:, :Lc], b[:, :Lc])      # the same chirps
    body_a, body_b = (r[:, Lc:].reshape(2, 2 * P + D, S) for r in (a, b))
    pil = list(range(P)) + list(range(P + D, 2 * P + D))
    assert same_bytes(body_a[:, pil], body_b[:, pil]) and not same_bytes(body_a[:, P:P + D], body_b[:, P:P + D])
    assert rep["data_peak"] == np.abs(body_a[:, P:P + D]).max()
    for tr, s in ((tx, sig), (ref, plain)):
        with contextlib.redirect_stdout(io.StringIO()):
            out = tr.receive(np.concatenate([np.zeros(2000), s, np.zeros(2000)]))[0]
        assert np.array_equal(out[: len(message)], message)
    tx.body_gain = 10.0 ** (rep["headroom_db"] / 20.0)                  # spend the headroom: the body now peaks where the chirp does
    np.random.seed(23)
    with contextlib.redirect_stdout(io.StringIO()):
        loud = tx.transmit(message)
        out = tx.receive(np.concatenate([np.zeros(2000), loud, np.zeros(2000)]))[0]
    assert np.array_equal(out[: len(message)], message)
    assert abs(tx.last_tx_report["headroom_db"]) <= 1e-9 and tx.last_tx_report["data_peak"] == pytest.approx(tx.body_gain * rep["data_peak"], rel=1e-12)
