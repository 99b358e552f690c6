"""Impulse noise, host side (no GPU): the packet interleaver's permutation, the carrier x symbol weights of the NumPy
restatement (tests/impulse_ref.py), and what the pair buys with the restated decoder (tests/ldpc_ref.py)."""
from math import gcd

import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import impulse_ref as IR
from tests import ldpc_ref as R
from tests import noise_ref as NR

PTS, BITS = orc.qpsk_table()
D, C, MU = 180, 1400, 2                                    # mode A2: one packet = 328 codewords of 1536 bits
# data carriers of the nine modes (lowest_bin .. highest_bin - 1 of the façade's table)
MODE_CARRIERS = {"A1": 2046, "A2": 1400, "A3": 900, "B1": 2046, "B2": 1400, "B3": 900, "C1": 2046, "C2": 1400, "C3": 900}


@pytest.mark.parametrize("geometry", sorted(MODE_CARRIERS) + ["odd"])
def test_permutation_is_a_bijection_with_the_smallest_coprime_stride(geometry):
    d, c, mu = (7, 9, 3) if geometry == "odd" else (180, MODE_CARRIERS[geometry], 2)
    nbp, B = d * c * mu, c * mu
    s = IR.stride(B, nbp)
    assert s >= B + 1 and gcd(s, nbp) == 1
    assert all(gcd(t, nbp) != 1 for t in range(B + 1, s))
    if geometry == "A2":
        assert s == 2801
    pi = IR.perm(d, c, mu)
    assert pi.shape == (nbp,) and np.array_equal(np.sort(pi), np.arange(nbp))
    assert pi[0] == 0 and pi[1] == s % nbp and pi[-1] == ((nbp - 1) * s) % nbp        # (the last product passes 2^31 in modes A1, B1, C1)
    x = np.random.default_rng(nbp).integers(0, 256, size=(2, nbp), dtype=np.uint8)
    y = IR.interleave(x, d, c, mu)
    assert np.array_equal(y[:, pi], x) and np.array_equal(IR.deinterleave(y, d, c, mu), x)
    assert not np.array_equal(y, x)
    if geometry != "odd":
        # consecutive coded bits land in consecutive symbols: a codeword keeps 8-9 bits in each of the 180 symbols
        sym = pi[:1536] // B
        assert np.array_equal(sym[1:180], sym[:179] + 1)
        assert set(np.bincount(sym, minlength=d).tolist()) <= {8, 9}


def impulse_failures(rate, sigma, sigma_bad, bad, seed=1, iters=20):
    """One packet of codewords over the unit-energy QPSK table plus noise of sigma per component on every symbol and
    sigma_bad on the whole symbols `bad`.  -> failed codewords for (stream order, per-carrier weights), (stream order, carrier x symbol),
    (interleaved, per-carrier), (interleaved, carrier x symbol)"""
    from gf3_audio_modem_amd.ldpc import shift_table
    sh = shift_table(rate)
    k = (sh.shape[1] - sh.shape[0]) * 64
    rng = np.random.default_rng(seed)
    nbp = D * C * MU
    n_cw = nbp // 1536
    msg = rng.integers(0, 2, size=(n_cw, k), dtype=np.uint8)
    stream = rng.integers(0, 2, size=nbp, dtype=np.uint8)                  # (the fill behind the last codeword: coin flips)
    stream[: n_cw * 1536] = R.encode(sh, msg).reshape(-1)
    lut = np.zeros(4, dtype=np.int64)
    lut[BITS[:, 0] * 2 + BITS[:, 1]] = np.arange(4)
    sig = np.full((D, 1), float(sigma))
    sig[list(bad)] = sigma_bad
    noise = (rng.normal(size=(D, C)) + 1j * rng.normal(size=(D, C))) * sig
    out = []
    for interleaved in (False, True):
        sent = IR.interleave(stream, D, C, MU) if interleaved else stream
        b = sent.reshape(D, C, MU)
        eq = PTS[lut[b[..., 0] * 2 + b[..., 1]]] + noise
        v_c, v_s = IR.noise_estimate2(eq, PTS, D)
        for llr in (NR.soft_demap_nw(eq, v_c, PTS, BITS, D), IR.soft_demap_nw2(eq, v_c, v_s, PTS, BITS)):
            if interleaved:
                llr = IR.deinterleave(llr, D, C, MU)
            bits, _, it = R.decode(sh, llr[: n_cw * 1536].reshape(n_cw, 1536), iters)
            out.append(int(np.sum((bits != msg).any(axis=1) | (it < 0))))
    return out


@pytest.mark.parametrize("rate,sigma,sigma_bad,bad", [("1/2", 0.35, 3.0, (60, 61, 62)), ("3/4", 0.25, 3.0, (60, 61, 62)),
                                                      ("1/2", 0.45, 5.0, (20, 21, 22, 100, 101, 102))])
def test_interleaver_and_symbol_weights_only_work_as_a_pair(rate, sigma, sigma_bad, bad):
    """Seed 1, 328 codewords, 20 iterations, the bad symbols' sigma at x0.8 / x1 / x1.2.  Three whole symbols are 8400
    adjacent coded bits: five to six codewords in stream order, whatever the weights; spread by the interleaver without a
    mark they poison most codewords; spread AND marked (weight ~ 1 / v_s) they cost every codeword 25 near-erasures of 1536."""
    for m in (0.8, 1.0, 1.2):
        stream_c, stream_cs, inter_c, inter_cs = impulse_failures(rate, sigma, sigma_bad * m, bad)
        print(f"rate {rate} sigma {sigma} / {sigma_bad * m:.2f} on {len(bad)} symbols: failed of 328 -- stream order {stream_c} | "
              f"{stream_cs} (per-carrier | carrier x symbol), interleaved {inter_c} | {inter_cs}")
        assert stream_c > 0
        assert inter_c > stream_c
        assert stream_cs > 0
        assert inter_cs == 0


# ---- the cases of tests/test_impulse_gpu.py::test_carrier_counts and ::test_every_arm_of_the_estimate -----------------
# launch_noise_cs turns C into NCG = 4, 8, 12 or 16 (the least of them >= ncg = (ceil(C / 64) + 1) // 2) and the table class
# into HI = 0 .. 3: sixteen kernels.  COUNTS sits on every boundary of that rule, on odd column counts and on one column.
COUNTS = [1, 64, 65, 129, 512, 513, 1024, 1025, 1536, 1537, 2047, 2048]
# HI = 0, 0, 1, 2, 3.  The reference's QPSK carries its FIRST label bit on the Q axis, so it is no binary-indexed grid in the
# sense of sep_is_binary (csrc/gf3rx_demap.h) and takes HI = 0 with the per-axis branch of the "any table" emitter; ring8
# takes HI = 0 with the literal scan; the binary-indexed 4-point grid (oracle.square_qam_table(2)) is what selects HI = 1.
ARM_TABLES = ["ring8", "qpsk_ref", "qam4", "qam16", "qam64"]
ARM_COUNTS = [65, 513, 1025, 1537]                                     # NCG = 4, 8, 12, 16
D_SMALL, F_SMALL = 3, 2


def arm_table(name):
    from tests import tables as T
    return orc.square_qam_table({"qam4": 2, "qam16": 4}[name]) if name in ("qam4", "qam16") else T.TABLES[name]


def ncg_arm(C):
    """The NCG template argument launch_noise_cs picks (None: refused)."""
    ncg = (-(-C // 64) + 1) // 2
    return next((a for a in (4, 8, 12, 16) if ncg <= a), None)


def grid_bits(points, bits):
    """grid_bits of csrc/gf3rx_demap.h restated: h for a 2^h x 2^h grid (h <= 3) whose first h label bits are the binary
    index of the I level and whose last h bits that of the Q level, levels numbered in order of appearance; else 0."""
    points, bits = np.asarray(points, dtype=complex), np.asarray(bits)
    M, mu = bits.shape
    li, lq = list(dict.fromkeys(points.real)), list(dict.fromkeys(points.imag))
    h = mu // 2
    if mu % 2 or h > 3 or len(li) != 1 << h or len(lq) != 1 << h or M != 1 << mu or len(set(points.tolist())) != M:
        return 0
    lab = (bits * (1 << np.arange(mu - 1, -1, -1))).sum(axis=1)
    want = [(li.index(z.real) << h) | lq.index(z.imag) for z in points]
    return h if lab.tolist() == want else 0


def count_case(table, C, scattered=False):
    """-> (parameter block, eq [F D, C]): points of the table plus noise whose level differs from carrier to carrier, with
    one symbol in five three times louder.  N = 4096 while the carriers fit, the top C bins or C bins drawn at random."""
    from tests import tables as T
    pts, bits = arm_table(table)
    N = 4096 if C <= 2047 else 8192
    K = N // 2 - 1
    bins = np.random.default_rng(C).permutation(K)[:C] + 1 if scattered else np.arange(K - C, K) + 1
    p = T.params_for((pts, bits), N, bins, P=1, D=D_SMALL, CP=0)
    rng = np.random.default_rng(1000 * len(pts) + C)
    idx = rng.integers(0, len(pts), size=(F_SMALL * D_SMALL, C))
    dmin = np.abs(pts[:, None] - pts[None, :])[np.triu_indices(len(pts), 1)].min()
    sig = dmin * (0.05 + 0.15 * rng.random(C)) * (1.0 + 2.0 * (rng.random((F_SMALL * D_SMALL, 1)) < 0.2))
    return p, pts[idx] + (rng.normal(size=idx.shape) + 1j * rng.normal(size=idx.shape)) * sig


def arm_cases():
    """(table, C, scattered): every (HI, NCG) pair, a scattered map at least once per NCG and per table."""
    return [(t, C, i % 4 == j) for i, t in enumerate(ARM_TABLES) for j, C in enumerate(ARM_COUNTS)]


def test_the_arm_cases_select_all_sixteen_kernels():
    assert [grid_bits(*arm_table(t)) for t in ARM_TABLES] == [0, 0, 1, 2, 3]
    assert [ncg_arm(C) for C in ARM_COUNTS] == [4, 8, 12, 16]
    arms = {(grid_bits(*arm_table(t)), ncg_arm(C)) for t, C, _ in arm_cases()}
    assert len(arms) == 16 and {ncg_arm(C) for t, C, s in arm_cases() if s} == {4, 8, 12, 16}
    # COUNTS: both sides of every boundary of the rule, the last accepted count, the first refused one
    assert [ncg_arm(C) for C in COUNTS] == [4, 4, 4, 4, 4, 8, 8, 12, 12, 16, 16, 16] and ncg_arm(2049) is None
    assert {-(-C // 64) % 2 for C in COUNTS} == {0, 1}                 # odd column counts: the second half is one column short


@pytest.mark.parametrize("C", COUNTS)
def test_count_cases_are_neither_flat_nor_erased(C):
    """What the GPU test's comparison rests on, by the restatement alone: every variance is finite and positive (no packet
    takes the flat rule, no weight is an erasure or the floor's), and every LLR of the reference is finite."""
    tables = ["qpsk_ref"] + ([t for t, c, _ in arm_cases() if c == C] if C in ARM_COUNTS else [])
    for table in dict.fromkeys(tables):
        for scattered in {False} | {s for t, c, s in arm_cases() if (t, c) == (table, C)}:
            p, eq = count_case(table, C, scattered)
            assert eq.shape == (F_SMALL * D_SMALL, C) and p.C == C and p.D == D_SMALL
            v_c, v_s = IR.noise_estimate2(eq, p.const_points, p.D)
            assert np.isfinite(v_c).all() and np.isfinite(v_s).all() and v_c.min() > 0 and v_s.min() > 0
            # (one carrier: v_c v_s / vbar = v_s, so the floor could bind only below 1e-6 of the packet's mean)
            x = v_c[:, None, :] * v_s[:, :, None] / v_c.mean(axis=1)[:, None, None]
            assert (x > 1e-6 * v_c.mean(axis=1)[:, None, None]).all()
            assert np.isfinite(IR.soft_demap_nw2(eq, v_c, v_s, p.const_points, p.const_bits)).all()


def test_nan_symbol_erases_that_symbol_only_and_a_noiseless_packet_gets_weight_one():
    rng = np.random.default_rng(4)
    Dn, Cn = 6, 40
    idx = rng.integers(0, 4, size=(3 * Dn, Cn))
    eq = PTS[idx].copy()                                                   # packet 0: noiseless
    eq[Dn:] += (rng.normal(size=(2 * Dn, Cn)) + 1j * rng.normal(size=(2 * Dn, Cn))) * 0.05
    eq[Dn + 2, 9] = complex(np.nan, 0.0)                                   # packet 1: one NaN sample
    eq[2 * Dn + 3, :] += (rng.normal(size=Cn) + 1j * rng.normal(size=Cn)) * 0.2     # packet 2: one loud symbol
    v_c, v_s = IR.noise_estimate2(eq, PTS, Dn)
    assert v_c.shape == (3, Cn) and v_s.shape == (3, Dn)
    np.testing.assert_array_equal(v_c, NR.noise_estimate(eq, PTS, Dn))
    w = IR.weights2(v_c, v_s)
    assert w.shape == (3, Dn, Cn)
    assert np.array_equal(w[0], np.ones((Dn, Cn)))                         # noiseless: weight 1, no division by zero
    # the NaN marks its carrier through v_c (as before) and its symbol through v_s: that symbol and that carrier are
    # erased and nothing else is -- the packet's mean being NaN, the rest falls back to weight 1
    assert np.isnan(v_s[1, 2]) and np.isfinite(np.delete(v_s[1], 2)).all()
    assert np.isnan(v_c[1, 9]) and np.isfinite(np.delete(v_c[1], 9)).all()
    want = np.ones((Dn, Cn))
    want[2, :] = 0.0
    want[:, 9] = 0.0
    assert np.array_equal(w[1], want)
    llr = IR.soft_demap_nw2(eq, v_c, v_s, PTS, BITS).reshape(3, Dn, Cn, 2)
    assert np.isfinite(llr).all() and not llr[1, 2].any() and not llr[1, :, 9].any()
    assert np.delete(np.delete(llr[1], 2, axis=0), 9, axis=1).all()
    np.testing.assert_allclose(llr[0], NR.maxlog(eq[:Dn], PTS, BITS), rtol=1e-6)
    # packet 2: the definition, element by element, and the loud symbol's smaller weight
    vbar = v_c[2].mean()
    np.testing.assert_allclose(w[2], 1.0 / np.maximum(np.outer(v_s[2], v_c[2]) / vbar, 1e-6 * vbar), rtol=1e-15)
    assert w[2, 3].mean() < 0.2 * np.delete(w[2], 3, axis=0).mean()
    snr = IR.symbol_snr_db(v_c, v_s, PTS)
    assert snr.shape == (3, Dn) and np.argmin(snr[2]) == 3 and np.isinf(snr[0]).all()
    np.testing.assert_allclose(snr[2], 10 * np.log10(1.0 / v_s[2]), rtol=1e-12)
    # the mean over the symbols of v_s and over the carriers of v_c are the same number
    assert np.mean(v_s[2]) == pytest.approx(np.mean(v_c[2]), rel=1e-12)
