"""Receive diversity, host side (no GPU): the NumPy restatement (tests/diversity_ref.py) against the single-branch
restatement it generalises, the declared interface, the façade's refusals, and the two-microphone scenario of DESIGN §12
with the oracle's receive chain and the restated decoder (tests/ldpc_ref.py)."""
import os
import re

import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import diversity_ref as DR
from tests import ldpc_ref as R
from tests import noise_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTS, BITS = orc.qpsk_table()
LEVEL_DB = 13.0                                            # noise below the RMS of the transmitted stream (nominal)


def test_one_branch_is_the_noise_weighted_demapper():
    """B = 1, noise weights: W is noise_ref.weights and the LLRs are noise_ref.soft_demap_nw's, bit for bit -- on symbols
    and variances that are dyadic rationals, so that (w z) / w is z exactly (with general values the combined symbol is z
    to one rounding, which the second half bounds); guards included: a NaN symbol, a NaN variance, a flat packet."""
    rng = np.random.default_rng(5)
    Dn, Cn, F = 6, 40, 3
    idx = rng.integers(0, 4, size=(F * Dn, Cn))
    eq = (np.round(PTS[idx] * 64) + rng.integers(-40, 41, size=idx.shape) + 1j * rng.integers(-40, 41, size=idx.shape)) / 64.0
    var = 2.0 ** rng.integers(-6, 3, size=(F, Cn)).astype(np.float64)
    var[1] = 0.0                                           # a flat packet: weights 1
    var[2, 7] = np.nan                                     # -> weight 0 there, and (the mean being NaN) 1 elsewhere
    eq[2 * Dn + 1, 9] = complex(np.nan, 0.0)
    z, W, llr = DR.combine_noise([eq], [var], Dn, PTS, BITS)
    w1 = np.repeat(NR.weights(var), Dn, axis=0)
    want = NR.soft_demap_nw(eq, var, PTS, BITS, Dn).reshape(F * Dn, Cn, 2)
    ok = np.isfinite(eq)
    assert np.array_equal(W[ok], w1[ok]) and W[2 * Dn + 1, 9] == 0.0 and z[2 * Dn + 1, 9] == 0.0
    assert np.array_equal(z[ok & (w1 > 0)], eq[ok & (w1 > 0)]) and not z[w1 == 0].any()
    got = llr.reshape(F * Dn, Cn, 2)
    assert np.array_equal(got[ok], want[ok]) and not got[2 * Dn + 1, 9].any() and not got[2 * Dn: 3 * Dn, 7].any()
    # general values: z to one rounding of the product and one of the quotient
    eq = PTS[idx] + (rng.normal(size=idx.shape) + 1j * rng.normal(size=idx.shape)) * 0.2
    var = NR.noise_estimate(eq, PTS, Dn)
    z, W, llr = DR.combine_noise([eq], [var], Dn, PTS, BITS)
    assert np.array_equal(W, np.repeat(NR.weights(var), Dn, axis=0))
    np.testing.assert_allclose(z, eq, rtol=4 * np.finfo(np.float64).eps)
    np.testing.assert_allclose(llr, NR.soft_demap_nw(eq, var, PTS, BITS, Dn), rtol=1e-6, atol=1e-9 * np.abs(llr).max())


def test_interface_is_declared():
    """gf3_combine_branches and GF3_MAX_BRANCHES: in the header, in the ctypes table, in the build's unit list."""
    from gf3_audio_modem_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gf3rx.h")).read()
    assert re.search(r"\bint\s+gf3_combine_branches\s*\(", hdr)
    m = re.search(r"#define\s+GF3_MAX_BRANCHES\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 4 == _lib.GF3_MAX_BRANCHES
    assert "gf3_combine_branches" in _lib.exported_names()
    assert "gf3rx_combine" in build.UNITS
    assert (_lib.GF3_COMBINE_CSI, _lib.GF3_COMBINE_NOISE) == tuple(
        int(re.search(rf"#define\s+{n}\s+(\d+)", hdr).group(1)) for n in ("GF3_COMBINE_CSI", "GF3_COMBINE_NOISE"))


def test_facade_refuses_without_gpu():
    from gf3_audio_modem_amd.OFDM import receiver
    x = np.zeros(1000)

    def rx(**attrs):
        r = receiver("A2", encoding=attrs.pop("encoding", "QCLDPC-5/6"), packet_length=20)
        for k, v in attrs.items():
            setattr(r, k, v)
        return r
    for signals in ([], [x] * 5, np.zeros((5, 100)), np.zeros((0, 100))):
        with pytest.raises(ValueError, match="1 to 4 recordings"):
            rx().receive_diversity(signals)
    with pytest.raises(ValueError, match="2-D array"):
        rx().receive_diversity(x)
    with pytest.raises(ValueError, match="noise2d"):
        rx(llr_weighting="noise2d").receive_diversity([x, x])
    with pytest.raises(ValueError, match="llr_weighting"):
        rx(llr_weighting="flat").receive_diversity([x, x])
    for name, value in (("fused_llr", True), ("phase_tracking", True), ("decoder_feedback", 1)):
        with pytest.raises(ValueError, match=name):
            rx(**{name: value}).receive_diversity([x, x])
    with pytest.raises(NotImplementedError, match="impulse_blanking"):
        rx(impulse_blanking=True).receive_diversity([x, x])
    with pytest.raises(NotImplementedError, match="plots"):
        rx().receive_diversity([x, x], graph_output=True)
    with pytest.raises(NotImplementedError, match="piece-wise"):
        rx(host_chunk_samples=1 << 20).receive_diversity([x, x])
    with pytest.raises(ValueError, match="interleave"):
        rx(encoding="None", interleave=True).receive_diversity([x, x])
    r = rx()
    assert r.last_branch_starts is None and r.last_branch_snr_db is None


def scenario():
    """Mode A2, packet_length 20, rate 5/6: one packet of 36 seeded codewords (and 704 seeded filler bits) through the
    oracle's synthesiser with a constant filler -> (parameter block, shift table, messages, coded bits, clean stream)"""
    from gf3_audio_modem_amd.ldpc import shift_table
    from gf3_audio_modem_amd.OFDM import receiver
    known = np.asarray(receiver("A2", packet_length=20).known_sequence, dtype=np.uint8)
    p = orc.RxParams(N=4096, CP=224, P=20, D=20, lo=100, hi=1500, const_points=PTS, const_bits=BITS, known_bits=known)
    sh = shift_table("5/6")
    k = (sh.shape[1] - sh.shape[0]) * 64
    rng = np.random.default_rng(7)
    msg = rng.integers(0, 2, size=(36, k), dtype=np.uint8)
    coded = np.concatenate([R.encode(sh, msg).reshape(-1), rng.integers(0, 2, size=p.D * p.C * 2 - 36 * 1536, dtype=np.uint8)])
    tx = orc.tx_stream(coded, np.full(p.K - p.C, (1 + 1j) / np.sqrt(2)), p, lead=300, tail=400)
    return p, sh, msg, coded, tx


def test_two_microphones_decode_what_neither_does_alone():
    """h0 = d[n] + 0.9 d[n-12]; h1 = d[n] - 0.9 d[n-17], 5 samples late; white noise (seeds 10, 11) 13 dB below the RMS of
    the transmitted stream, amplitude x0.8 / x1.0 / x1.2; the oracle's receive (its own sync per branch), 50 iterations.
    Failed codewords of 36, branch 0 alone (csi | noise), branch 1 alone (csi | noise), combined (csi | noise); raw BER
    of branch 0, branch 1 -> combined (csi):
        x0.8 (14.9 dB):   9 | 11    8 | 11    0 | 0    4.5 %, 4.5 % -> 0.7 %
        x1.0 (13 dB):    32 | 31   34 | 36    0 | 0    5.9 %, 5.9 % -> 1.1 %
        x1.2 (11.4 dB):  36 | 36   36 | 36    0 | 0    7.3 %, 7.3 % -> 1.6 %
    The plain average of the two branches' symbols fails all 36 at every level: the weights are the feature."""
    p, sh, msg, coded, tx = scenario()
    clean = DR.two_paths(tx)
    for scale in (0.8, 1.2, 1.0):
        outs = [orc.receive(b, p) for b in DR.add_noise(clean, tx, LEVEL_DB, scale)]
        assert [o["starts"].tolist() for o in outs] == [[300 + p.Lc], [300 + p.Lc + DR.DELAY]]
        eqs = [o["eq"] for o in outs]
        raw = [float(np.mean(o["bits"] != coded)) for o in outs]
        vars_ = [NR.noise_estimate(e, PTS, p.D) for e in eqs]
        zc, _, llr_c = DR.combine_csi(eqs, [o["Hs"] for o in outs], [o["He"] for o in outs], p.data_carriers, p.P, p.D, PTS, BITS)
        zn, _, llr_n = DR.combine_noise(eqs, vars_, p.D, PTS, BITS)
        raw_c = [float(np.mean(BITS[NR.decide(z, PTS)].reshape(-1) != coded)) for z in (zc, zn)]
        comb = [DR.failed(sh, llr, msg) for llr in (llr_c, llr_n)]
        print(f"x{scale}: raw BER {raw[0]:.4f} {raw[1]:.4f} -> combined {raw_c[0]:.4f} (csi) {raw_c[1]:.4f} (noise); "
              f"combined failed {comb[0]} (csi) {comb[1]} (noise)")
        assert max(raw) < 0.15                              # every branch is locked
        assert max(raw_c) < min(raw)
        assert comb == [0, 0]
        if scale == 1.0:
            alone = [[DR.failed(sh, DR.single_llrs(o, w, p), msg) for w in ("csi", "noise")] for o in outs]
            plain = DR.failed(sh, NR.maxlog((eqs[0] + eqs[1]) / 2, PTS, BITS).astype(np.float32).reshape(-1), msg)
            print(f"x{scale}: alone failed (csi, noise) {alone[0]} {alone[1]}; plain average failed {plain}")
            assert min(min(a) for a in alone) >= 1
            assert plain >= 1


def test_noise_weights_follow_the_branch_that_is_clean():
    """Planted variances: two branches carry the same symbols, branch 1 with 9x the noise variance on the upper half of
    the carriers.  W there is 1/v0 + 1/(9 v0) to the estimate's accuracy, a noiseless branch dominates a noisy one
    (weight 1e6 / vbar against 1 / v), and the SNR rows are those of the definition."""
    rng = np.random.default_rng(12)
    Dn, Cn, F = 64, 96, 2
    idx = rng.integers(0, 4, size=(F * Dn, Cn))
    n0, n1 = ((rng.normal(size=(2,) + idx.shape) + 1j * rng.normal(size=(2,) + idx.shape)) * np.sqrt(0.002 / 2))
    n1[:, Cn // 2:] *= 3.0
    eqs = [PTS[idx] + n0, PTS[idx] + n1]
    vars_ = [NR.noise_estimate(e, PTS, Dn) for e in eqs]
    z, W, _ = DR.combine_noise(eqs, vars_, Dn, PTS, BITS)
    hi = W[:, Cn // 2:].reshape(F, Dn, -1)[:, 0]
    # each estimate is chi-square with 2 D degrees of freedom: relative standard deviation 1 / sqrt(D), 5 sigma
    assert np.abs(hi / (1 / 0.002 + 1 / 0.018) - 1.0).max() < 5.0 / np.sqrt(Dn)
    np.testing.assert_allclose(W.reshape(F, Dn, Cn)[:, 0], 1 / vars_[0] + 1 / vars_[1], rtol=1e-14)
    assert np.mean(np.abs(z - PTS[idx])[:, Cn // 2:] ** 2) < 0.0021          # below branch 0's own 0.002 x (1 + margin)
    np.testing.assert_allclose(DR.combined_snr_db(vars_, PTS), 10 * np.log10(1 / vars_[0] + 1 / vars_[1]), rtol=1e-12)
    np.testing.assert_allclose(DR.branch_snr_db(vars_, PTS)[1], NR.snr_db(vars_[1], PTS), rtol=1e-12)
    assert (DR.combined_snr_db(vars_, PTS) > DR.branch_snr_db(vars_, PTS)).all()
    # a noiseless branch 0
    z, W, _ = DR.combine_noise([PTS[idx], eqs[1]], [np.zeros((F, Cn)), vars_[1]], Dn, PTS, BITS)
    assert np.isfinite(W).all() and np.abs(z - PTS[idx]).max() < 1e-4
