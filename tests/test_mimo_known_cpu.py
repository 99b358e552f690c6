"""The known-bit joint detector and the cancellation loop, host side (no GPU): the declared interface, the façade's
refusals and default, the NumPy restatement (tests/mimo_known_ref.py) against mimo_ref's detector and against the
single-stream limit computed on its own, and the case DESIGN §12 ("Cancelling decoded streams") reports: the worth of the
feature in the scenario's room, restated on the CPU.  tests/test_mimo_known_gpu.py holds the kernel to the same restatement."""
import os
import re

import numpy as np
import pytest

from tests import crc_ref as CR
from tests import ldpc_ref as R
from tests import mimo_known_ref as KR
from tests import mimo_ref as MR
from tests.test_mimo_cpu import small_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The settled case (searched on the CPU: levels 11.5 .. 0 dB, noise seeds (s, s + 100) with s in 0 .. 29; the list is in DESIGN §12)
LEVEL_DB = 3.0
SEEDS = (18, 118)
FIRST, LEFT, PASSES = 2, 0, 1                               # untrusted codewords of 10 after the first decode, at the end; passes run
SLIP = 5e-3                                                 # |slope| beyond this is the fit's slip (1e-4 .. 3e-3 without, 2e-2 and more with)


def test_interface_is_declared():
    from gf3_audio_modem_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gf3rx.h")).read()
    assert re.search(r"\bint\s+gf3_mimo_detect_known\s*\(", hdr)
    assert "gf3_mimo_detect_known" in _lib.exported_names()
    res, args = _lib._SIGS["gf3_mimo_detect_known"]
    assert len(args) == 11                                  # ctx, B, Y, H, slope, w, bits, known, F, llr, stream
    m = re.search(r"#define\s+GF3_LLR_KNOWN\s+(\S+)", hdr)
    assert m and m.group(1) == "1e30f"
    assert np.float32(m.group(1).rstrip("f")) == np.float32(_lib.GF3_LLR_KNOWN) == KR.LLR_KNOWN
    assert np.isfinite(np.float32(_lib.GF3_LLR_KNOWN))


def test_facade_refuses_without_gpu_and_defaults():
    from gf3_audio_modem_amd.coding import CodedChain
    from gf3_audio_modem_amd.OFDM import receiver
    x = np.zeros(1000)

    def rx(encoding="QCLDPC-1/2", **attrs):
        r = receiver("A2", encoding=encoding, no_pilots=20, packet_length=20)
        for k, v in attrs.items():
            setattr(r, k, v)
        return r
    assert rx().mimo_cancellation == 0 and receiver("A3").mimo_cancellation == 0
    assert rx()._chain().mimo_cancellation == 0 and rx(mimo_cancellation=3)._chain().cancellation() == 3
    assert CodedChain.__dataclass_fields__["mimo_cancellation"].default == 0
    for bad in (-1, 1.5, True, None, "2", [1]):
        with pytest.raises(ValueError, match="mimo_cancellation must be an integer >= 0"):
            rx(mimo_cancellation=bad).receive_mimo([x, x])
        with pytest.raises(ValueError, match="mimo_cancellation must be an integer >= 0"):
            rx(mimo_cancellation=bad).receive_stbc([x])
    for encoding in ("None", "XOR"):
        with pytest.raises(ValueError, match="receive_mimo: mimo_cancellation needs a 'QCLDPC-\\*' encoding"):
            rx(encoding, mimo_cancellation=1).receive_mimo([x, x])
    for encoding in ("QCLDPC-1/2", "None"):
        with pytest.raises(ValueError, match="receive_stbc: mimo_cancellation.*nothing to cancel"):
            rx(encoding, mimo_cancellation=2).receive_stbc([x])
    # an existing refusal of plan_mimo stays in front of it
    with pytest.raises(ValueError, match="decoder_feedback"):
        rx(mimo_cancellation=1, decoder_feedback=1).receive_mimo([x, x])
    with pytest.raises(NotImplementedError, match="impulse_blanking"):
        rx(mimo_cancellation=1, impulse_blanking=True).receive_mimo([x, x])


# ---- the restated detector ---------------------------------------------------------------------------------------------
def inputs(p, F, B, seed):
    """tests/test_mimo_gpu.py's detect_inputs: random spectra, estimates whose end block differs from the start block, slopes"""
    rng = np.random.default_rng(seed)
    cn = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    Ys = [cn(F * p.D, p.N // 2 + 1) for _ in range(B)]
    Hs = []
    for _ in range(B):
        H = cn(F, 2, 2, p.K) * 0.7
        H[:, 1] = H[:, 0] * (1 + 0.3 * rng.normal(size=(F, 2, p.K))) * np.exp(0.2j * rng.normal(size=(F, 2, p.K)))
        Hs.append(H)
    return Ys, Hs, [3e-3 * rng.normal(size=F) for _ in range(B)]


def noiseless(p, F, B, seed):
    """Random estimates and sent points x0, x1 [F, D, C]; Y_b = h_b0 x0 + h_b1 x1 exactly on the data carriers' bins
    -> (Ys, Hs, slopes, the sent table indices [F, 2, D, C])"""
    Ys, Hs, slopes = inputs(p, F, B, seed)
    idx = np.random.default_rng(seed + 1).integers(0, 4, size=(F, 2, p.D, p.C))
    x = np.asarray(p.const_points)[idx]
    for Y, H, s in zip(Ys, Hs, slopes):
        h0, h1 = MR.channel_entries(H, s, p)
        Y.reshape(F, p.D, -1)[:, :, p.data_carriers] = h0 * x[:, 0] + h1 * x[:, 1]
    return Ys, Hs, slopes, idx


def brute(stats, cell, p, bits, known):
    """One cell (f, l, c) by two loops over the points, straight from the rule: -> the four LLRs [2, mu]"""
    G00, G11, G01, m0, m1, live = (v[cell] for v in stats)
    pts, lab = np.asarray(p.const_points), np.asarray(p.const_bits)
    f, l, c = cell
    out = np.zeros((2, 2))
    for s in range(2):
        for q in range(2):
            if known[f, s, l, c, q]:
                out[s, q] = -1e30 if bits[f, s, l, c, q] else 1e30
                continue
            best = {0: np.inf, 1: np.inf}
            for i in range(4):
                for j in range(4):
                    if any(known[f, t, l, c, r] and bool(bits[f, t, l, c, r]) != bool(lab[(i, j)[t], r]) for t in range(2) for r in range(2)):
                        continue
                    d = (G00 * abs(pts[i]) ** 2 + G11 * abs(pts[j]) ** 2 + 2.0 * (np.conj(pts[i]) * G01 * pts[j]).real
                         - 2.0 * (np.conj(pts[i]) * m0).real - 2.0 * (np.conj(pts[j]) * m1).real)
                    v = int(lab[(i, j)[s], q])
                    best[v] = min(best[v], d)
            out[s, q] = (best[1] - best[0]) if live else 0.0
    return out


def test_nothing_known_is_the_plain_detector():
    p = small_params(P=2)
    for B in (1, 2, 4):
        Ys, Hs, slopes = inputs(p, 2, B, 40 + B)
        Ys[0][3, p.data_carriers[7]] = complex(np.nan, 0.0)
        ref, _ = MR.detect(Ys, Hs, slopes, p)
        zero = np.zeros(ref.shape, dtype=np.uint8)
        for bits in (zero, np.full_like(zero, 1)):
            got = KR.detect_known(Ys, Hs, slopes, p, bits, zero)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_stream_0_known_leaves_stream_1_its_own_column():
    """x0 known as sent: stream 1's LLRs are the single-stream max-log LLRs of z = m1 - conj(G01) x0 under the gain G11,
    min over x with the bit 1 of G11 |x|^2 - 2 Re(conj(x) z) less the same with the bit 0 -- computed here from the
    sufficient statistics, without the pair metric."""
    p = small_params(P=2)
    Ys, Hs, slopes, idx = noiseless(p, 2, 2, 5)
    rng = np.random.default_rng(6)
    for Y in Ys:                                                # (noise, so that the LLRs are not those of an exact fit)
        Y += 0.3 * (rng.normal(size=Y.shape) + 1j * rng.normal(size=Y.shape))
    lab, pts = np.asarray(p.const_bits), np.asarray(p.const_points)
    bits = lab[idx].astype(np.uint8)                            # [F, 2, D, C, mu]
    known = np.zeros_like(bits)
    known[:, 0] = 1
    got = KR.llrs_known(Ys, Hs, slopes, p, bits, known)
    G00, G11, G01, m0, m1, live = MR.sufficient(Ys, Hs, slopes, p)
    assert live.all()
    z = m1 - np.conj(G01) * pts[idx[:, 0]]
    cost = G11[..., None] * np.abs(pts) ** 2 - 2.0 * (np.conj(pts) * z[..., None]).real        # [F, D, C, 4]
    want = np.stack([cost[..., lab[:, q] == 1].min(axis=-1) - cost[..., lab[:, q] == 0].min(axis=-1) for q in range(2)], axis=-1)
    print(f"stream 1 under a known stream 0: worst relative deviation {np.abs(got[:, 1] / want - 1).max():.2e}")
    # rtol 1e-12 on every LLR.  An LLR is a difference of two costs, and both computations round the costs, not the
    # difference: near a tie (|LLR| below 1e-4 of the costs) a relative bound on the difference asks for more than float64
    # holds -- measured, one LLR of 7900, 6.8e-5 in size, deviates by 8.3e-17.  So beside it an absolute floor of 1e-15 of the
    # largest cost, a few units in its last place; for every other element the relative bound is the larger of the two.
    np.testing.assert_allclose(got[:, 1], want, rtol=1e-12, atol=1e-15 * np.abs(cost).max())
    assert np.array_equal(got[:, 0], np.where(bits[:, 0] != 0, -1e30, 1e30).astype(np.float32).astype(np.float64))
    # and it helps: the plain detector decides stream 1 wrongly somewhere, the informed one at fewer cells
    plain = MR.detect(Ys, Hs, slopes, p)[0]
    wrong_plain = int(((plain[:, 1] < 0) != (bits[:, 1] != 0)).sum())
    wrong_known = int(((got[:, 1] < 0) != (bits[:, 1] != 0)).sum())
    print(f"stream 1 bit errors: plain {wrong_plain}, stream 0 known {wrong_known} of {bits[:, 1].size}")
    assert wrong_known < wrong_plain


def test_a_contradicting_known_bit_moves_the_other_stream():
    """The mask is not vacuous: noiseless, with x0 declared to be the point of the complemented label, stream 1's decision
    is the best x1 beside that WRONG x0 -- it leaves the sent x1 at many cells -- and the brute-force scan agrees."""
    p = small_params(P=2)
    Ys, Hs, slopes, idx = noiseless(p, 1, 2, 9)
    lab = np.asarray(p.const_bits)
    sent = lab[idx].astype(np.uint8)
    zero = np.zeros_like(sent)
    plain = KR.detect_known(Ys, Hs, slopes, p, zero, zero)
    assert np.array_equal(plain < 0, sent != 0)                # noiseless: the joint argmin is what was sent
    bits, known = sent.copy(), zero.copy()
    bits[:, 0] ^= 1
    known[:, 0] = 1
    got = KR.detect_known(Ys, Hs, slopes, p, bits, known)
    moved = ((got[:, 1] < 0) != (sent[:, 1] != 0)).any(axis=-1)
    print(f"stream 1 decisions moved by a contradicting stream 0: {int(moved.sum())} of {moved.size} cells")
    assert moved.mean() > 0.25
    stats = MR.sufficient(Ys, Hs, slopes, p)
    for cell in [tuple(c) for c in np.argwhere(moved[0])[:5]] + [(0, 0, 0), (0, p.D - 1, p.C - 1)]:
        want = brute(stats, (0,) + tuple(cell[-2:]), p, bits, known)
        np.testing.assert_allclose(got[0, :, cell[-2], cell[-1]], want.astype(np.float32), rtol=1e-6)


def test_one_bit_of_a_point_known():
    """Cells with one bit of a point known and the other not, in every combination over the two streams (a random mask of
    single bits): the unknown bit's two sets hold the pairs that agree with the known one.  Against the brute-force scan."""
    p = small_params(P=2)
    Ys, Hs, slopes = inputs(p, 1, 3, 12)
    rng = np.random.default_rng(13)
    shape = (1, 2, p.D, p.C, 2)
    bits = rng.integers(0, 2, size=shape).astype(np.uint8)
    known = (rng.random(size=shape) < 0.5).astype(np.uint8)
    got = KR.detect_known(Ys, Hs, slopes, p, bits, known)
    assert np.isfinite(got).all()
    stats = MR.sufficient(Ys, Hs, slopes, p)
    kinds = set()
    for l in range(p.D):
        for c in range(0, p.C, 7):
            kinds.add(tuple(known[0, :, l, c].reshape(-1)))
            want = brute(stats, (0, l, c), p, bits, known).astype(np.float32)
            np.testing.assert_allclose(got[0, :, l, c], want, rtol=1e-6, atol=0)
    assert len(kinds) == 16                                     # every pattern of known bits over the cell's four was met
    # a known bit never changes the sign the other bits' LLRs would need to contradict it: known LLRs are exact
    assert np.array_equal(got[known != 0], np.where(bits[known != 0] != 0, -KR.LLR_KNOWN, KR.LLR_KNOWN))


# ---- the worth of the feature ------------------------------------------------------------------------------------------
def coded_scenario(pairs=2):
    """small_params' geometry with P = 4 and D = 5 (N = 1024, CP = 64, C = 395): `pairs` packet pairs of 7900 coded bits each,
    holding 10 seeded rate-1/2 codewords with their CRC and 440 seeded fill bits, constant filler, the scenario's room
    -> (p, shift table, messages, the speakers' streams, clean recordings)"""
    from gf3_audio_modem_amd.ldpc import shift_table
    p = small_params(P=4, D=5)
    sh = shift_table("1/2")
    k = (sh.shape[1] - sh.shape[0]) * R.Z
    total = pairs * 2 * p.D * p.C * p.mu
    n_cw = total // 1536
    rng = np.random.default_rng(7)
    msg = CR.attach(rng.integers(0, 2, size=(n_cw, k - 32), dtype=np.uint8), k)
    coded = np.concatenate([R.encode(sh, msg).reshape(-1), rng.integers(0, 2, size=total - n_cw * 1536, dtype=np.uint8)])
    tx2 = MR.tx_mimo(coded, np.full(p.K - p.C, (1 + 1j) / np.sqrt(2)), p, lead=300, tail=400)
    return p, sh, msg, tx2, MR.through(tx2)


def test_cancellation_recovers_codewords_in_the_room():
    """"QCLDPC-1/2" with the codeword CRC over the scenario's room, window advance 16, white noise LEVEL_DB below a packet
    body (seeds SEEDS), the restated chain with the restated decoder, 50 iterations, 10 codewords in two packet pairs.
    Measured: 2 codewords fail the first decode; with mimo_cancellation = 2 one pass is run, both come back (0 left) and
    every message row is the sent one.  No slope has slipped (largest |slope| 3.1e-3 rad per carrier; a slip is 2e-2 and
    more): a packet whose slope has slipped is lost whatever the detector does."""
    p, sh, msg, tx2, clean = coded_scenario()
    assert len(msg) == 10
    rec = KR.add_noise(clean, tx2, LEVEL_DB, SEEDS)
    res, o = KR.receive(rec, p, sh, len(msg), 2, crc=True, advance=16)
    worst = max(float(np.abs(s).max()) for s in o["slopes"])
    print(f"{LEVEL_DB} dB, seeds {SEEDS}: untrusted after the first decode {res['first']}, after cancellation {res['left']}, "
          f"passes {res['passes']}, trusted in pass {res['trusted_in'].tolist()}, largest |slope| {worst:.2e}")
    assert worst < SLIP
    assert 1 <= res["first"] < len(msg)
    assert (res["first"], res["left"], res["passes"]) == (FIRST, LEFT, PASSES)
    assert res["first"] - res["left"] >= 1
    assert np.array_equal(res["msg"], msg) and not res["bad"].any()
    # without the option the loop is the plain chain: the same first-pass failures, nothing more
    off = KR.loop(o["llr"], None, sh, len(msg), 2 * p.D * p.C * p.mu, 0, crc=True)
    assert (off["first"], off["left"], off["passes"]) == (FIRST, FIRST, 0)
