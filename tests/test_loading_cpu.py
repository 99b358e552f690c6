"""Adaptive bit loading without a GPU: the allocation rule, the layout and the mapper against the restatement
(tests/loading_ref.py), the table's validation, what the façade and the coded chain refuse, and the ABI's declarations."""
import os
import re

import numpy as np
import pytest

from tests import loading_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def patterns(C=130):
    """The loadings the GPU tests use (tests/test_loading_gpu.py imports them from here)."""
    mixed = np.zeros(C, dtype=np.uint8)
    mixed[:63] = 2
    mixed[63], mixed[64], mixed[65] = 6, 0, 4
    mixed[66:128] = np.resize([0, 2, 4, 6], 62)
    mixed[128], mixed[129] = 0, 6
    # first and last carrier off; a run of 70 zeros, carriers 58 .. 127: both kernels put carriers 64 k .. 64 k + 63 into one
    # wave, so the wave of carriers 64 .. 127 holds zeros only (the estimate takes nothing but the pilot loop there, the
    # demapper stores nothing)
    zeros = np.resize([6, 4, 2], C).astype(np.uint8)
    zeros[0] = zeros[-1] = 0
    zeros[58:128] = 0
    assert not zeros[64:128].any() and zeros[57] and zeros[128]
    return {"mixed": mixed, "zeros": zeros, "all2": np.full(C, 2, np.uint8), "all4": np.full(C, 4, np.uint8),
            "all6": np.full(C, 6, np.uint8), "single": np.array([6], dtype=np.uint8),
            "cycle": np.resize([0, 2, 4, 6], 170).astype(np.uint8)}


# ---- allocation ---------------------------------------------------------------------------------------------------
def test_allocation_thresholds_cap_nonfinite_minimum_and_monotony():
    from gf3_audio_modem_amd.loading import bit_loading_from_snr
    for gap in (0.0, 3.0, 8.8):
        for b, lin in ((2, 3.0), (4, 15.0), (6, 63.0)):
            t = 10 * np.log10(lin) + gap
            got = bit_loading_from_snr(np.array([t - 0.01, t + 0.01]), gap_db=gap)
            assert got.dtype == np.uint8 and got.tolist() == [b - 2, b], (gap, b, got)
    snr = np.array([-5.0, 4.0, 5.0, 11.0, 12.0, 17.0, 19.0, 40.0])
    assert bit_loading_from_snr(snr, gap_db=0.0).tolist() == [0, 0, 2, 2, 4, 4, 6, 6]
    assert bit_loading_from_snr(snr, gap_db=0.0, max_bits=4).tolist() == [0, 0, 2, 2, 4, 4, 4, 4]
    assert bit_loading_from_snr(snr, gap_db=0.0, max_bits=2).tolist() == [0, 0, 2, 2, 2, 2, 2, 2]
    assert bit_loading_from_snr(snr, gap_db=0.0, max_bits=0).tolist() == [0] * 8
    assert bit_loading_from_snr(np.array([np.nan, np.inf, -np.inf, 30.0]), gap_db=0.0).tolist() == [0, 0, 0, 6]
    # [F, C]: the per-carrier minimum over the packets; a non-finite entry in any packet switches the carrier off
    two = np.array([[30.0, 30.0, 13.0, 30.0], [30.0, 6.0, 30.0, np.nan]])
    assert bit_loading_from_snr(two, gap_db=0.0).tolist() == [6, 2, 4, 0]
    ramp = np.linspace(-10, 50, 601)
    assert (np.diff(bit_loading_from_snr(ramp, gap_db=4.0).astype(int)) >= 0).all()
    with pytest.raises(TypeError):
        bit_loading_from_snr(ramp)                                  # gap_db has no default
    with pytest.raises(ValueError):
        bit_loading_from_snr(np.zeros((2, 2, 2)), gap_db=1.0)


# ---- layout, mapper ---------------------------------------------------------------------------------------------------
def test_layout_of_hand_written_tables():
    from gf3_audio_modem_amd.loading import loading_layout
    Bs, off = loading_layout(np.array([2, 0, 6, 4, 0, 2], dtype=np.uint8))
    assert Bs == 14 and off.tolist() == [0, 2, 2, 8, 12, 12, 14]
    Bs, off = loading_layout(np.full(200, 6, dtype=np.uint8))       # (no uint8 overflow)
    assert Bs == 1200 and off[-2] == 1194
    for order in patterns().values():
        Bs, off = loading_layout(order)
        assert (Bs, off.tolist()) == (LR.layout(order)[0], LR.layout(order)[1].tolist()) and not (off % 2).any()


def test_tables_are_the_engines_and_the_stated_levels():
    """The restatement's levels are the stated quotient; square_qam_table's differ from them by one rounding at most (its
    complex division by the real scale is a multiplication by the reciprocal), and its labels are the same."""
    from gf3_audio_modem_amd.engine import square_qam_table
    for m in (2, 4, 6):
        pts, bits = square_qam_table(m)
        rp, rb = LR.table(m)
        assert np.array_equal(bits, rb)
        assert max(np.abs(pts.real - rp.real).max(), np.abs(pts.imag - rp.imag).max()) <= 2.0 ** -52 and abs(np.mean(np.abs(rp) ** 2) - 1.0) < 1e-15
        assert (np.arange(1 << m) == (bits << np.arange(m - 1, -1, -1)).sum(axis=1)).all()
        # the host mapper sends exactly square_qam_table's points, label by label (what the library's levels are held to)
        from gf3_audio_modem_amd.loading import map_loaded
        sent = map_loaded(bits.reshape(-1), np.array([m], dtype=np.uint8), np.zeros(1, dtype=complex))[:, 0]
        assert np.array_equal(sent.view(np.int64), pts.view(np.int64))
    # the all-2 family is not the reference's QPSK table: there the first label bit lies on the Q axis
    from gf3_audio_modem_amd.engine import qpsk_table
    q_pts, q_bits = qpsk_table()
    s_pts, s_bits = square_qam_table(2)
    first = lambda pts, bits, axis: all(len({(pts[i].real, pts[i].imag)[axis] for i in range(4) if bits[i, 0] == v}) == 1 for v in (0, 1))
    assert first(s_pts, s_bits, 0) and first(q_pts, q_bits, 1) and not first(q_pts, q_bits, 0)


@pytest.mark.parametrize("name", list(patterns()))
def test_mapper_round_trip_and_pilot_points(name):
    from gf3_audio_modem_amd.loading import loading_layout, map_loaded
    order = patterns()[name]                                   # every table the GPU cases use
    C, n = len(order), 5
    rng = np.random.default_rng(len(name))
    known = np.exp(2j * np.pi * rng.random(C))
    Bs, off = loading_layout(order)
    bits = rng.integers(0, 2, size=n * Bs)
    sym = map_loaded(bits, order, known)
    assert sym.shape == (n, C) and sym.dtype == np.complex128
    np.testing.assert_allclose(sym, LR.map_loaded(bits, order, known), rtol=0, atol=2.0 ** -51)      # (one rounding per axis)
    assert np.array_equal(sym[:, order == 0], np.tile(known[order == 0], (n, 1)))
    assert np.array_equal(LR.hard_bits(LR.soft_demap(sym, order, n)), bits)           # unit weights, noiseless
    assert np.allclose(LR.noise_estimate(sym, order, known, n), 0.0, atol=1e-30)


def test_validation():
    from gf3_audio_modem_amd.loading import validate_loading
    ok = validate_loading([0, 2, 4, 6], 4)
    assert ok.dtype == np.uint8 and ok.tolist() == [0, 2, 4, 6]
    for bad, C in (([2, 3, 4], 3), ([2, 8, 4], 3), ([2, 4], 3), ([0, 0, 0], 3), ([[2, 4, 6]], 3), ([2.5, 4, 6], 3), ([-2, 4, 6], 3)):
        with pytest.raises(ValueError, match="bit_loading"):
            validate_loading(bad, C)


# ---- façade and coded chain ---------------------------------------------------------------------------------------
def a2_order():
    order = np.zeros(1400, dtype=np.uint8)
    order[:500], order[500:900], order[900:1300] = 6, 4, 2
    return order


def test_facade_sizes_and_unchanged_chain_without_a_loading():
    from gf3_audio_modem_amd.coding import CodedChain
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2", encoding="QCLDPC-1/2", no_pilots=4, packet_length=8)
    assert rx.bit_loading is None and rx.loaded_bits_per_symbol == rx.data_bits_per_symbol == 2800
    chain = rx._chain()
    today = CodedChain(rx.encoding, rx.ldpc_n, rx.ldpc_max_iter, rx.llr_weighting, rx.interleave, rx.fused_llr, rx.outer_code,
                       per_packet=8 * 2800, make_code=chain.make_code, codeword_crc=False, phase_tracking=False,
                       decoder_feedback=0, feedback_window=(2, 8), feedback_min_known=4)
    assert chain == today and chain.loading is None and chain.rate() == "1/2"
    rx.bit_loading = a2_order()
    assert rx.loaded_bits_per_symbol == 500 * 6 + 400 * 4 + 400 * 2 == 5400
    assert (rx.mu, rx.data_bits_per_symbol, rx.bits_per_symbol) == (2, 2800, 4094)
    chain = rx._chain()
    assert chain.per_packet == 8 * 5400 and chain.loading == tuple(a2_order().tolist()) and chain.rate() == "1/2"
    assert chain.check_receive() == ("1/2", False)
    assert chain.outer_layout(2) == (2 * 8 * 5400 // 1536, 0)
    rx.encoding = "None"
    assert rx._chain().rate() is None


def test_refusals_under_a_loading_need_no_gpu():
    from gf3_audio_modem_amd.OFDM import receiver

    def fresh(**kw):
        rx = receiver("A2", encoding="QCLDPC-1/2", no_pilots=4, packet_length=8)
        rx.bit_loading = a2_order()
        for k, v in kw.items():
            setattr(rx, k, v)
        return rx
    sig = np.zeros(4096)
    for kw in (dict(interleave=True), dict(llr_weighting="noise2d"), dict(fused_llr=True), dict(phase_tracking=True),
               dict(decoder_feedback=1), dict(encoding="XOR")):
        rx = fresh(**kw)
        for call in (rx._chain().check_receive, rx._chain().rate, rx._qcldpc_rate, lambda: rx.receive(sig),
                     lambda: rx.encode(np.zeros(10, dtype=np.int64))):
            with pytest.raises(ValueError, match="bit_loading"):
                call()
    for table in (np.full(1399, 2), np.full(1400, 3), np.full(1400, 8), np.zeros(1400, dtype=int)):
        rx = fresh(bit_loading=table)
        for call in (lambda: rx._chain().check_receive(), lambda: rx._chain().rate(), lambda: rx.receive(sig),
                     lambda: rx.loaded_bits_per_symbol, lambda: rx.transmit(np.zeros(10, dtype=np.int64))):
            with pytest.raises(ValueError, match="bit_loading"):
                call()
    with pytest.raises(ValueError, match="bit_loading"):
        fresh().receive_diversity([sig, sig])
    with pytest.raises(NotImplementedError, match="bit_loading"):
        fresh().receive(sig, graph_output=True)
    rx = fresh()
    rx.host_chunk_samples = 1 << 20
    with pytest.raises(NotImplementedError, match="bit_loading.*piece-wise host path"):
        rx.receive(sig)
    # without a loading none of this changed: the same settings pass the chain's checks
    rx = receiver("A2", encoding="QCLDPC-1/2")
    rx.interleave, rx.llr_weighting = True, "noise2d"
    assert rx._chain().check_receive() == ("1/2", False)


def test_encode_fills_loaded_packets():
    """encoding "None" runs on the host: the coin-flip fill completes a packet of packet_length * Bs bits."""
    from gf3_audio_modem_amd.OFDM import transmitter
    tx = transmitter("A2", encoding="None", no_pilots=4, packet_length=8)
    tx.bit_loading = a2_order()
    np.random.seed(1)
    bits = np.arange(50_000) % 2
    out = tx.encode(bits)
    assert len(out) == 2 * 8 * 5400 and np.array_equal(out[:50_000], bits)


# ---- ABI ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_loading_calls_and_the_binding_knows_them():
    from gf3_audio_modem_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gf3rx.h")).read()
    declared = set(re.findall(r"\b(gf3_[a-z_]+)\s*\(", hdr))
    new = {"gf3_loading_create", "gf3_loading_destroy", "gf3_loading_bits", "gf3_noise_estimate_loaded", "gf3_soft_demap_loaded"}
    assert new <= declared and new <= set(_lib.exported_names())
    assert "typedef struct gf3_loading gf3_loading;" in hdr
