"""Decoder feedback on the GPU: gf3_feedback_equalise against the NumPy restatement (tests/feedback_ref.py) on the smallest
shapes at which the kernel can go wrong, its calling conventions and refusals, the loop of CodedChain.decode_feedback
against the restated loop on engine-produced symbols, and `decoder_feedback` end to end through the façade on a packet
under a moving echo.

Tolerances.  The gain is a ratio of two sums of at most 17 x 129 terms; the two sides add the same terms in different
orders, each within (terms) x 2^-53 of sum |r|, i.e. 2.5e-13 S with S = sum |r| / B: |g - g_ref| <= 1e-12 S.  Where the
restatement counts fewer than min_known known symbols the gate is an integer comparison: g == 1 exactly, no case left
out.  out against eq / g, with the kernel's own g: one complex division, 1e-14 |out|.  Measured on the MI355X on the rows
added for MU = 1, 4, 5, 7 and 8: |g - g_ref| / S 1.9e-16 .. 5.9e-16, |out - eq / g| / |out| 1.2e-16 .. 4.1e-16."""
import functools

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import crc_ref as CR
from tests import feedback_ref as FB
from tests import ldpc_ref as R
from tests import noise_ref as NR
from tests import tables as T

pytestmark = pytest.mark.gpu
TABLES = {"qpsk": orc.qpsk_table(), "qam16": orc.square_qam_table(4), "qam64": orc.square_qam_table(6),
          "ring8": T.TABLES["ring8"], "tri3": T.TABLES["tri3"], "bpsk": T.TABLES["bpsk"], "cross32": T.TABLES["cross32"],
          "ring8_mu7": T.TABLES["ring8_mu7"], "grid16_mu8": T.TABLES["grid16_mu8"]}


def bins_of(kind, C):
    """contig: C bins from 100 on; descending: the same, listed downwards; comb3 (every third bin) and shuffled (scattered
    bins in a random order): the first C carriers of the map of tests/tables.py at K = 2047."""
    if kind in ("contig", "descending"):
        bins = np.arange(100, 100 + C)
        return bins if kind == "contig" else bins[::-1].copy()
    bins = T.MAPS[kind](2047)
    assert len(bins) >= C
    return bins[:C].copy()


@functools.lru_cache(maxsize=None)
def _engine(table, bins, D):
    from gf3_audio_modem_amd import Engine, RxConfig
    pts, bits = TABLES[table]
    mu = np.asarray(bits).shape[1]
    N = 4096
    return Engine(RxConfig(N=N, CP=0, P=1, D=D, data_bins=np.asarray(bins), const_points=np.asarray(pts),
                           const_bits=np.asarray(bits).astype(np.int64), known_bits=np.zeros((N // 2 - 1) * mu, np.uint8),
                           in_dtype=torch.float64, fit_lo=10, fit_hi=100))


def engine_of(table, bins, D):
    return _engine(table, tuple(int(b) for b in bins), D)


def synth(table, bins, F, D, density, seed, wrong=0.1, plant=True):
    """Random points of the table under a smooth per-carrier, per-symbol gain plus noise; `bits` their labels, a tenth of them
    replaced by random labels (wrong reference symbols are the caller's business, not the kernel's); a random symbol mask
    of `density`; a non-finite symbol planted at a known and at an unknown position where there is one."""
    pts, tb = TABLES[table]
    rng = np.random.default_rng(seed)
    C, mu = len(bins), tb.shape[1]
    idx = rng.integers(0, len(pts), size=(F * D, C))
    l = (np.arange(F * D) % D)[:, None]
    gain = (1 + 0.4 * np.sin(l / 3 + np.asarray(bins)[None, :] / 50)) * np.exp(0.5j * np.cos(l / 5 - np.asarray(bins)[None, :] / 70))
    eq = pts[idx] * gain + 0.05 * (rng.normal(size=idx.shape) + 1j * rng.normal(size=idx.shape))
    other = rng.integers(0, len(pts), size=idx.shape)
    bits = tb[np.where(rng.random(size=idx.shape) < wrong, other, idx)].astype(np.uint8).reshape(-1)
    sym = rng.random(size=(F * D, C)) < density
    if plant and eq.size > 2:
        flat = eq.reshape(-1)
        for where, value in ((np.flatnonzero(sym.reshape(-1)), complex(np.nan, 0.3)), (np.flatnonzero(~sym.reshape(-1)), complex(-0.2, np.inf))):
            if len(where):
                flat[where[len(where) // 2]] = value
    return eq, bits, np.repeat(sym.astype(np.uint8), mu)


def compare(case, table, bins, D, eq, bits, known, hs, hb, min_known):
    pts, tb = TABLES[table]
    eng = engine_of(table, bins, D)
    _, g_ref, n, S = FB.feedback(eq, bits, known, pts, tb, bins, D, hs, hb, min_known)
    out, g = eng.feedback_equalise(eq, torch.from_numpy(bits), torch.from_numpy(known), hs, hb, min_known, want_gain=True)
    assert out.dtype == torch.complex128 and tuple(out.shape) == eq.shape and g.dtype == torch.complex128 and tuple(g.shape) == eq.shape
    out, g = out.cpu().numpy(), g.cpu().numpy()
    gate = n >= min_known
    assert (g[~gate] == 1).all(), f"{case}: a gain used on fewer than min_known known symbols"
    e_g = (np.abs(g - g_ref)[gate] / np.maximum(S[gate], 1e-300)).max(initial=0.0)
    fin = np.isfinite(eq.real) & np.isfinite(eq.imag)
    assert np.isfinite(g.real).all() and np.isfinite(g.imag).all()
    assert np.array_equal(np.isfinite(out.real) & np.isfinite(out.imag), fin), f"{case}: non-finite symbols"
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        want = eq / g
        e_out = (np.abs(out - want)[fin] / np.abs(out)[fin]).max(initial=0.0)
    one = g == 1
    assert np.array_equal(out[one].view(np.float64), eq[one].view(np.float64), equal_nan=True), f"{case}: g = 1 must copy eq"
    print(f"{case}: C {eq.shape[1]} D {D} F {eq.shape[0] // D} window ({hs}, {hb}) min_known {min_known}: gate open on {int(gate.sum())} of "
          f"{gate.size}, |g - g_ref| / S {e_g:.2e} (1e-12), |out - eq / g| / |out| {e_out:.2e} (1e-14)")
    assert e_g <= 1e-12 and e_out <= 1e-14
    return out, g, n


# table, map, C, D, F, half_symbols, half_bins, density, min_known
CASES = [
    ("qpsk", "contig", 1400, 5, 3, 2, 8, 0.3, 4),              # the default window on the reference's band: 11 carrier tiles
    ("qpsk", "contig", 1400, 2, 1, 8, 64, 0.3, 4),             # both halves at their largest, half_symbols >= D
    ("qpsk", "contig", 1400, 40, 1, 1, 1, 1.0, 4),             # five symbol tiles
    ("qam16", "contig", 65, 40, 3, 1, 1, 0.3, 3),              # one carrier past half a tile; windows of 9 around min_known
    ("qam16", "contig", 65, 5, 1, 0, 64, 0.3, 4),
    ("qam64", "contig", 64, 40, 1, 8, 64, 1.0, 4),             # every symbol known, every window as large as the packet allows
    ("qam64", "contig", 64, 2, 3, 1, 0, 0.3, 1),               # half_bins = 0: the carrier's own column
    ("qam64", "shuffled", 65, 5, 3, 2, 8, 0.3, 4),
    ("ring8", "contig", 7, 1, 3, 0, 0, 1.0, 1),                # D = 1, the window is the symbol itself
    ("ring8", "contig", 7, 5, 1, 8, 1, 0.3, 2),
    ("ring8", "comb3", 64, 5, 3, 1, 64, 0.3, 4),
    ("ring8", "descending", 65, 2, 1, 0, 1, 1.0, 2),
    ("qpsk", "contig", 1, 1, 1, 0, 0, 1.0, 1),                 # one carrier, one symbol
    ("qpsk", "contig", 1, 5, 3, 1, 64, 0.3, 1),
    ("qpsk", "contig", 1, 40, 1, 8, 0, 1.0, 4),
    ("qpsk", "shuffled", 650, 1, 1, 0, 8, 0.3, 2),             # scattered bins over six tiles: the halo is sparse
    ("qpsk", "descending", 1400, 2, 3, 1, 64, 0.3, 4),
    ("qpsk", "comb3", 600, 5, 1, 2, 1, 1.0, 1),                # bins three apart, half_bins = 1: every window one column wide
    ("qam16", "comb3", 7, 40, 3, 8, 8, 0.0, 1),                # nothing known
    ("qpsk", "contig", 65, 5, 3, 2, 8, 0.0, 4),
    ("qam64", "descending", 7, 2, 1, 1, 1, 0.3, 1),
    ("tri3", "contig", 65, 5, 1, 1, 8, 1.0, 2),                # a label no point carries (bits drawn from all four below)
    # every launch_feedback<MU>, MU = 1 .. 8, on a map that is not contiguous (MU 2, 3, 6: above), and one carrier past a tile
    ("bpsk", "shuffled", 64, 5, 3, 2, 8, 0.3, 2),              # MU = 1
    ("bpsk", "contig", 65, 2, 1, 1, 1, 1.0, 1),
    ("qam16", "shuffled", 65, 5, 3, 1, 8, 0.3, 2),             # MU = 4 with known symbols (the comb3 row above knows none)
    ("cross32", "comb3", 64, 5, 3, 2, 8, 0.3, 4),              # MU = 5: byte-wise label loads of an odd width
    ("cross32", "descending", 65, 5, 1, 1, 64, 0.3, 2),
    ("ring8_mu7", "shuffled", 64, 5, 3, 2, 8, 0.3, 4),         # MU = 7: a 128-entry label table for 8 points
    ("ring8_mu7", "comb3", 65, 3, 2, 1, 1, 1.0, 1),
    ("grid16_mu8", "comb3", 64, 5, 3, 2, 8, 0.3, 4),           # MU = 8: 8-byte label loads, a 256-entry label table for 16 points
    ("grid16_mu8", "shuffled", 65, 5, 1, 8, 64, 0.3, 2),       # both halves at their largest: the LDS planes at their widest
    ("grid16_mu8", "contig", 65, 5, 1, 1, 8, 1.0, 2),          # labels no point carries (bits drawn from all 256 below)
]
ANY_LABEL = [("tri3", "contig"), ("grid16_mu8", "contig")]      # rows whose bits are drawn from every label, carried or not


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_kernel_against_the_restatement(case):
    table, kind, C, D, F, hs, hb, density, min_known = case
    bins = bins_of(kind, C)
    eq, bits, known = synth(table, bins, F, D, density, seed=len(kind) + 7 * C + D)
    if (table, kind) in ANY_LABEL:
        bits = np.random.default_rng(3).integers(0, 2, size=bits.shape, dtype=np.uint8)
    _, g, n = compare("-".join(str(v) for v in case), table, bins, D, eq, bits, known, hs, hb, min_known)
    if density == 0.0:
        assert not n.any() and (g == 1).all()
    if density == 1.0 and (table, kind) not in ANY_LABEL:
        assert (n >= 1).sum() >= n.size - 1                        # (all but the planted non-finite symbol's own window)


def test_masks_on_the_gate():
    """Three known symbols side by side, then a fourth: with min_known = 4 the gain is used exactly where the window holds all
    four; the same around a tile boundary of the carriers (128) and of the symbols (8)."""
    masks_on_the_gate("qpsk")


@pytest.mark.parametrize("table", ["ring8_mu7", "grid16_mu8"])
def test_masks_on_the_gate_with_the_widest_labels(table):
    """The same with 7 and 8 mask bytes per symbol: a symbol is known where all of them are set."""
    masks_on_the_gate(table)
    # one mask byte of the fourth symbol cleared, the first or the last: the symbol is not known, the gate stays shut
    bins = bins_of("contig", 200)
    D, mu = 12, TABLES[table][1].shape[1]
    eq, bits, _ = synth(table, bins, 1, D, 0.0, seed=5, wrong=0.0, plant=False)
    mask = np.zeros((D, len(bins)), dtype=bool)
    mask[2, 5] = mask[2, 6] = mask[3, 5] = mask[3, 7] = True
    for b in (0, mu - 1):
        known = np.repeat(mask.astype(np.uint8), mu).reshape(D, len(bins), mu)
        known[3, 7, b] = 0
        _, g, n = compare(f"gate_byte_{b}", table, bins, D, eq, bits, known.reshape(-1), 1, 2, 4)
        assert n.max() == 3 and (g == 1).all()


def masks_on_the_gate(table):
    bins = bins_of("contig", 200)
    D, mu = 12, TABLES[table][1].shape[1]
    for l0, c0 in ((2, 5), (7, 126), (6, 127)):
        eq, bits, _ = synth(table, bins, 1, D, 0.0, seed=c0, wrong=0.0, plant=False)
        mask = np.zeros((D, len(bins)), dtype=bool)
        mask[l0, c0] = mask[l0, c0 + 1] = mask[l0 + 1, c0] = True
        _, g, n = compare(f"gate_three_{c0}", table, bins, D, eq, bits, np.repeat(mask.astype(np.uint8), mu), 1, 2, 4)
        assert n.max() == 3 and (g == 1).all()
        mask[l0 + 1, c0 + 2] = True
        _, g, n = compare(f"gate_four_{c0}", table, bins, D, eq, bits, np.repeat(mask.astype(np.uint8), mu), 1, 2, 4)
        four = np.zeros_like(mask)
        four[l0: l0 + 2, c0: c0 + 3] = True
        assert np.array_equal(n == 4, four) and np.array_equal(g != 1, four)


# ---- calling conventions ----------------------------------------------------------------------------------------------
def test_repeatable_with_and_without_the_gain():
    bins = bins_of("contig", 1400)
    D, F = 7, 3
    eng = engine_of("qpsk", bins, D)
    eq, bits, known = (torch.from_numpy(a).cuda() for a in synth("qpsk", bins, F, D, 0.3, seed=77))
    out, g = eng.feedback_equalise(eq, bits, known, want_gain=True)
    again, g2 = eng.feedback_equalise(eq, bits, known, want_gain=True)
    for x, y in ((out, again), (g, g2)):
        assert x is not y and np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    alone = eng.feedback_equalise(eq, bits, known)
    assert isinstance(alone, torch.Tensor) and np.array_equal(alone.cpu().numpy().view(np.uint8), out.cpu().numpy().view(np.uint8))
    given = torch.empty(F * D * len(bins), dtype=torch.complex128, device="cuda")
    assert eng.feedback_equalise(eq, bits, known, out=given) is given
    assert np.array_equal(given.cpu().numpy().view(np.uint8), out.cpu().numpy().reshape(-1).view(np.uint8))
    # F = 0
    o0, g0 = eng.feedback_equalise(torch.empty((0, len(bins)), dtype=torch.complex128), torch.empty(0, dtype=torch.uint8),
                                   torch.empty(0, dtype=torch.uint8), want_gain=True)
    assert tuple(o0.shape) == (0, len(bins)) and tuple(g0.shape) == (0, len(bins))


def test_refusals():
    from gf3_audio_modem_amd import _lib
    bins = bins_of("contig", 65)
    D = 5
    eng = engine_of("qpsk", bins, D)
    eq, bits, known = (torch.from_numpy(a).cuda() for a in synth("qpsk", bins, 1, D, 0.3, seed=3))
    with pytest.raises(ValueError, match="eq"):
        eng.feedback_equalise(eq[:-1], bits, known)
    with pytest.raises(ValueError, match="bits must be uint8"):
        eng.feedback_equalise(eq, bits[:-1], known)
    with pytest.raises(ValueError, match="known must be uint8"):
        eng.feedback_equalise(eq, bits, known.to(torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        eng.feedback_equalise(eq, bits, known, out=torch.empty(eq.numel() - 1, dtype=torch.complex128, device="cuda"))
    with pytest.raises(ValueError, match="out must not be eq"):
        eng.feedback_equalise(eq, bits, known, out=eq)
    for kw in (dict(half_symbols=9), dict(half_symbols=-1), dict(half_bins=65), dict(half_bins=-1), dict(min_known=0), dict(half_bins=1.5)):
        with pytest.raises(ValueError, match="feedback"):
            eng.feedback_equalise(eq, bits, known, **kw)
    lib = _lib.load()
    out = torch.empty_like(eq)
    p, b, k, q = _lib.ptr(eq), _lib.ptr(bits), _lib.ptr(known), _lib.ptr(out)
    assert lib.gf3_feedback_workspace_bytes(eng._h, 1) == 0
    call = lambda ctx, p_, b_, k_, F, hs, hb, mk, q_, wb=0: lib.gf3_feedback_equalise(ctx, p_, b_, k_, F, hs, hb, mk, q_, None, None, wb, None)
    assert call(eng._h, p, b, k, 0, 2, 8, 4, q) == 0                     # F == 0: a no-op, whatever the pointers
    assert call(eng._h, None, None, None, 0, 2, 8, 4, None) == 0
    bad = {"no context": (None, p, b, k, 1, 2, 8, 4, q), "null pointer": (eng._h, None, b, k, 1, 2, 8, 4, q),
           "null pointer ": (eng._h, p, None, k, 1, 2, 8, 4, q), "null pointer  ": (eng._h, p, b, None, 1, 2, 8, 4, q),
           "null pointer   ": (eng._h, p, b, k, 1, 2, 8, 4, None), "d_out must not be d_eq": (eng._h, p, b, k, 1, 2, 8, 4, p),
           "F < 0": (eng._h, p, b, k, -1, 2, 8, 4, q), "half_symbols": (eng._h, p, b, k, 1, 9, 8, 4, q),
           "half_symbols ": (eng._h, p, b, k, 1, -1, 8, 4, q), "half_bins": (eng._h, p, b, k, 1, 2, 65, 4, q),
           "half_bins ": (eng._h, p, b, k, 1, 2, -1, 4, q), "min_known": (eng._h, p, b, k, 1, 2, 8, 0, q),
           "workspace too small": (eng._h, p, b, k, 1, 2, 8, 4, q, -1)}
    for text, args in bad.items():
        assert call(*args) == _lib.GF3_EINVAL, text
        msg = lib.gf3_last_error(None)
        assert b"gf3_feedback_equalise" in msg and text.strip().encode() in msg, (text, msg)
    assert call(eng._h, p, b, k, 1, 2, 8, 4, q) == 0                     # (no gain, no workspace)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint8), eng.feedback_equalise(eq, bits, known).cpu().numpy().view(np.uint8))


# ---- the loop, and the façade -----------------------------------------------------------------------------------------
P, D = 4, 12                               # mode A2 (C = 1400): 33 600 coded bits per packet, 21 codewords of 1536
ALPHA0, TAU, NOISE_DB, SEED = 0.9, 10, 14.0, 5
LEAD = 2000


@functools.lru_cache(maxsize=None)
def echo_streams():
    """One packet of "QCLDPC-1/2" with the per-codeword CRC, built on the host: 21 x 736 payload bits, CRC, the restated
    encoder, a random fill past the last codeword, the oracle's transmitter with a terminating chirp.
    -> (p, payload, start, the stream under the moving echo plus noise, the same noise on the clean stream)"""
    from gf3_audio_modem_amd.OFDM import receiver
    from gf3_audio_modem_amd.ldpc import shift_table
    rx = receiver("A2", encoding="QCLDPC-1/2", no_pilots=P, packet_length=D)
    pts, tb = orc.qpsk_table()
    p = orc.RxParams(N=4096, CP=224, P=P, D=D, lo=100, hi=1500, const_points=pts, const_bits=tb,
                     known_bits=np.asarray(rx.known_sequence[: rx.K * rx.mu], dtype=np.uint8))
    rng = np.random.default_rng(SEED)
    per = D * p.C * 2
    n_cw = per // 1536
    payload = rng.integers(0, 2, size=n_cw * 736, dtype=np.uint8)
    coded = rng.integers(0, 2, size=per, dtype=np.uint8)
    coded[: n_cw * 1536] = R.encode(shift_table("1/2"), CR.attach(payload.reshape(n_cw, 736), 768)).reshape(-1)
    fill = rng.choice(np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) / np.sqrt(2), size=p.K - p.C)
    sig = orc.tx_stream(coded, fill, p, lead=LEAD, tail=LEAD)
    start = LEAD + p.Lc
    body = sig[LEAD: len(sig) - LEAD - p.Lc]
    noise = rng.normal(0, np.sqrt(np.mean(body ** 2) / 10 ** (NOISE_DB / 10)), sig.shape)
    return p, payload, start, FB.moving_echo(sig, start, p.S, D, P, ALPHA0, TAU) + noise, sig + noise


def facade():
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2", encoding="QCLDPC-1/2", no_pilots=P, packet_length=D)
    rx.codeword_crc, rx.llr_weighting = True, "noise"
    return rx


def test_the_chain_loop_trusts_what_the_restated_loop_trusts():
    """On the symbols the engine's demodulator leaves of the echo stream: after p = 0 .. 3 passes CodedChain.decode_feedback
    trusts exactly the codewords the restated loop (restated noise weights, decoder, CRC and feedback) trusts by then."""
    from gf3_audio_modem_amd.ldpc import shift_table
    p, payload, start, noisy, _ = echo_streams()
    pts, tb = p.const_points, p.const_bits
    rx = facade()
    eng = rx._engine(np.dtype("float64"))
    o = eng.demod_frames(eng._samples(noisy), [start], want=("Hs", "He", "slope", "status", "eq"))
    eq = o["eq"].cpu().numpy()
    n_cw = D * p.C * 2 // 1536
    weigh = lambda e: NR.soft_demap_nw(e, NR.noise_estimate(e, pts, D), pts, tb, D)
    ref = FB.loop(eq, weigh, shift_table("1/2"), n_cw, pts, tb, p.data_carriers, D, 3, crc=True)
    print(f"restated: trusted in pass {ref['trusted_in'].tolist()}, {ref['passes']} passes")
    assert ref["passes"] >= 2 and (ref["trusted_in"] != 0).sum() >= 3 and (ref["trusted_in"] >= 0).all()
    code = rx._chain().code("1/2", eng.device)
    for passes in range(4):
        rx.decoder_feedback = passes
        chain = rx._chain()
        if passes == 0:
            bits, iters, _, bad = chain.decode(code, chain.llrs(eng, o, pts)[0])
            fb = {"feedback_passes": 0, "feedback_recovered": 0}
        else:
            bits, iters, _, bad, rows, fb = chain.decode_feedback(eng, code, o, pts)
            assert tuple(rows["last_snr_db"].shape) == (1, p.C)
        trusted = (iters.cpu().numpy() > 0) & (bad.cpu().numpy() == 0)
        want = (ref["trusted_in"] >= 0) & (ref["trusted_in"] <= passes)
        assert np.array_equal(trusted, want), (passes, trusted, ref["trusted_in"])
        assert fb == {"feedback_passes": min(passes, ref["passes"]), "feedback_recovered": int(want.sum() - (ref["trusted_in"] == 0).sum())}
        got = bits.cpu().numpy().reshape(n_cw, 736)
        assert np.array_equal(got[trusted], payload.reshape(n_cw, 736)[trusted])
        assert np.array_equal(iters.cpu().numpy()[trusted], ref["iters"][trusted])


def test_facade_decoder_feedback_decodes_a_packet_under_a_moving_echo():
    """Mode A2 with no_pilots = 4, packet_length = 12, "QCLDPC-1/2", codeword_crc, llr_weighting "noise", no interleaver: one
    packet of 21 codewords.  The stream passes through moving_echo(alpha0 = 0.9, tau = 10) and white noise 14 dB below the
    packet, seed 5.

    Chosen on the host with the restated chain (oracle demodulation, restated noise weights, decoder, CRC and feedback), whose
    counts of 21 codewords are: the first decode fails 8 (codewords 7 .. 14, the middle of the packet), pass 1 recovers 6,
    pass 2 the other 2, and the payload comes back.  At alpha0 x 1.1: 8 fail, 4 + 4 recovered in two passes; at noise
    x 1.1: 8 fail, 5 + 3 in two passes; the payload comes back both times.  With alpha0 = 0 every codeword decodes at once
    (also at noise x 1.1) and no pass runs."""
    p, payload, start, noisy, clean = echo_streams()
    rx = facade()
    assert rx.decoder_feedback == 0
    out, _, _ = rx.receive(noisy)
    rep = rx.last_decode_report
    print(f"without feedback: {rep['inner_failed']} of {rep['codewords']} failed: {rep['failed_codewords'].tolist()}")
    assert not np.array_equal(out[: len(payload)], payload)
    assert rep["inner_failed"] >= 3 and "feedback_passes" not in rep and "feedback_recovered" not in rep
    rx.decoder_feedback = 4
    out, Hs0, _ = rx.receive(noisy)
    rep = rx.last_decode_report
    print(f"with feedback: {rep['feedback_passes']} passes recovered {rep['feedback_recovered']}, {rep['inner_failed']} failed")
    assert out.dtype == np.int64 and Hs0.shape == (2047,)
    assert np.array_equal(out[: len(payload)], payload)
    assert rep["feedback_recovered"] >= 3 and rep["inner_failed"] == 0 and 1 <= rep["feedback_passes"] <= 4
    assert rep["codewords"] == 21 and rep["crc_failed"] == 0 and rx.last_snr_db.shape == (1, p.C)
    # a clean stream: no pass runs, and the bits are those of the receiver without feedback
    on, _, _ = rx.receive(clean)
    rep = rx.last_decode_report
    assert rep["feedback_passes"] == 0 and rep["feedback_recovered"] == 0 and rep["inner_failed"] == 0
    rx.decoder_feedback = 0
    off, _, _ = rx.receive(clean)
    assert np.array_equal(on, off) and np.array_equal(off[: len(payload)], payload)
    assert "feedback_passes" not in rx.last_decode_report
    # the refusals, before any GPU work
    rx.decoder_feedback, rx.fused_llr, rx.llr_weighting = 1, True, "csi"
    with pytest.raises(ValueError, match="decoder_feedback"):
        rx.receive(clean)
    from gf3_audio_modem_amd.OFDM import receiver
    other = receiver("A2", encoding="XOR", no_pilots=P, packet_length=D)
    other.decoder_feedback = 1
    with pytest.raises(ValueError, match="decoder_feedback"):
        other.receive(clean)
