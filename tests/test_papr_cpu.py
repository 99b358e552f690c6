"""Tone reservation without a GPU: the properties of the NumPy restatement (tests/papr_ref.py) on seeded symbols, the
validators, the façade's defaults and refusals (raised before any GPU work), and the keys of `last_tx_report`."""
import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import papr_ref as PR

K = 511
KNOWN = np.random.default_rng(1).integers(0, 2, size=2 * K).astype(np.uint8)


def small_params(carriers=None, lo=25, hi=376):
    pts, bt = orc.qpsk_table()
    return orc.RxParams(N=1024, CP=56, P=1, D=3, lo=lo, hi=hi, carriers=carriers, const_points=pts, const_bits=bt,
                        known_bits=KNOWN, fit_lo=64, fit_hi=256)


def scattered():
    """Every third carrier from 25 on and a block at the top: reserved carriers lie between data carriers."""
    return np.concatenate([np.arange(25, 376, 3), np.arange(400, 460)])


# Geometries that select the kernel instantiations and label widths the first six cases of tests/test_papr_gpu.py leave
# out: papr_kernel<1024> (N = 2048), papr_kernel<4096> (N = 8192, the arm with more than 64 KiB of dynamic LDS), and labels
# of 1, 3, 5, 7 and 8 bits through the kernel's own three-byte window (every width but 1 and 8 straddles bytes).
WIDTH_TABLES = ["bpsk", "psk8", "cross32", "ring8_mu7", "grid16_mu8"]
MORE_GEOMETRIES = ["n2048_contig", "n2048_scattered", "n8192_contig"] + WIDTH_TABLES


def more_params(name):
    """-> (parameters, packets) of one of MORE_GEOMETRIES."""
    from tests import tables as T
    if name == "n2048_contig":
        return T.params_for("qpsk_ref", 2048, np.arange(25, 700), P=1, D=3, CP=120), 3
    if name == "n2048_scattered":                                        # every third carrier and a block above them
        return T.params_for("qpsk_ref", 2048, np.concatenate([np.arange(25, 700, 3), np.arange(800, 900)]), P=1, D=3, CP=120), 3
    if name == "n8192_contig":
        return T.params_for("qpsk_ref", 8192, np.arange(100, 3000), P=1, D=2, CP=480), 2
    return T.params_for(name, 1024, np.arange(25, 376), P=1, D=3, CP=56), 3


def payload_bits(name, p, F):
    """The seed rule of tests/test_papr_gpu.py::case.  A table with fewer points than labels draws among the labels it
    carries (the oracle's mapper and tx_kernel differ, on purpose, on a label that no point carries)."""
    rng = np.random.default_rng(len(name) + 100)
    if len(p.const_points) < 1 << p.mu:
        return p.const_bits[rng.integers(0, len(p.const_points), size=F * p.D * p.C)].reshape(-1)
    return rng.integers(0, 2, size=F * p.D * p.C * p.mu)


@pytest.mark.parametrize("name", MORE_GEOMETRIES)
def test_more_geometries_leave_no_ties(name):
    """The condition under which tests/test_papr_gpu.py compares the best index as an integer: at most 1 % of the symbols
    have their two smallest iterate peaks within 1e-9 of each other, at I = 16 and I = 3, by the restatement alone."""
    p, F = more_params(name)
    bits = payload_bits(name, p, F)
    for iterations in (16, 3):
        tones, rep, peaks = PR.tone_reserve(bits, p, 6.0, 6.0, iterations)
        share = float(np.mean([PR.near_tie(q) for q in peaks]))
        print(f"{name} I={iterations}: N {p.N} C {p.C} mu {p.mu}: share of ties {share}, mean peak {rep[..., 0].mean():.4f} -> "
              f"{rep[..., 1].mean():.4f}, best index mean {rep[..., 2].mean():.1f}")
        assert tones.shape == (F, p.D, p.K - p.C) and share <= 0.01
        assert (rep[..., 2] > 0).any()                                   # (the iteration runs: some symbol is clipped)


@pytest.mark.parametrize("name", ["contig", "scattered"])
def test_restatement_properties(name):
    p = small_params() if name == "contig" else small_params(carriers=scattered())
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2, size=12 * p.D * p.C * p.mu)
    for limit_db in (6.0, -6.0):
        tones, rep, peaks = PR.tone_reserve(bits, p, 6.0, limit_db, 16)
        L = 10.0 ** (limit_db / 20.0)
        assert tones.shape == (12, p.D, p.K - p.C) and rep.shape == (12, p.D, 4)
        assert (rep[..., 1] <= rep[..., 0]).all()                        # never worse than a zero filler
        assert np.abs(tones).max() <= L * (1 + 1e-12)
        X = orc.map_bits(bits.reshape(-1, p.C, p.mu), p)
        for row, R, r, pk in zip(X, tones.reshape(-1, p.K - p.C), rep.reshape(-1, 4), peaks):
            x = PR.symbol(row, R, p)
            assert np.abs(x).max() == r[1] == pk[int(r[2])] == pk.min() and int(r[2]) == int(np.argmin(pk))
            assert r[0] == pk[0] == np.abs(PR.symbol(row, np.zeros_like(R), p)).max()
            assert r[3] == np.sqrt(np.mean(x ** 2))
        print(f"{name}, limit {limit_db} dB: mean peak {rep[..., 0].mean():.4f} -> {rep[..., 1].mean():.4f}, "
              f"mean best index {rep[..., 2].mean():.1f}")
        assert rep[..., 1].mean() < rep[..., 0].mean()                   # (and it does lower the peaks of random symbols)


def test_restatement_degenerate_cases():
    p = small_params()
    bits = np.random.default_rng(3).integers(0, 2, size=p.D * p.C * p.mu)
    tones, rep, peaks = PR.tone_reserve(bits, p, 6.0, 6.0, 0)                # I = 0: zero tones
    assert not tones.any() and (rep[..., 2] == 0).all() and (rep[..., 0] == rep[..., 1]).all() and all(len(q) == 1 for q in peaks)
    # a symbol already under A stops at index 0: no sample of a random symbol reaches 13 dB above the data's rms here
    tones, rep, peaks = PR.tone_reserve(bits, p, 13.0, 6.0, 16)
    X = orc.map_bits(bits.reshape(-1, p.C, p.mu), p)
    sigma = np.sqrt(2 * np.sum(np.abs(X) ** 2, axis=1)) / p.N
    assert (rep[0, :, 0] <= sigma * 10 ** (13 / 20)).all()               # (the condition on the inputs)
    assert not tones.any() and (rep[..., 2] == 0).all() and all(len(q) == 1 for q in peaks)
    assert PR.near_tie(np.array([1.0, 2.0, 1.0 + 1e-10])) and not PR.near_tie(np.array([1.0, 1.1])) and not PR.near_tie(np.array([1.0]))


def test_check_papr():
    from gf3_audio_modem_amd import Engine
    assert Engine.check_papr(6, np.float64(-3.0), np.int64(4)) == (6.0, -3.0, 4)
    for bad in (2.9, 13.1, float("nan"), float("inf"), "6", None, True):
        with pytest.raises(ValueError, match="papr target"):
            Engine.check_papr(bad, 6.0, 16)
    for bad in (-20.5, 21, float("nan"), float("-inf"), "6", None, False):
        with pytest.raises(ValueError, match="papr tone limit"):
            Engine.check_papr(6.0, bad, 16)
    for bad in (-1, 65, 4.0, "4", None, True):
        with pytest.raises(ValueError, match="papr iterations"):
            Engine.check_papr(6.0, 6.0, bad)


# ---- the façade: defaults, refusals before any GPU work, the report ---------------------------------------------------
def tx_of(mode="A2", **kw):
    from gf3_audio_modem_amd.OFDM import transmitter
    tx = transmitter(mode, encoding=kw.pop("encoding", "None"), no_pilots=2, packet_length=4)
    tx.papr_reduction = True
    for k, v in kw.items():
        setattr(tx, k, v)
    return tx


def test_facade_defaults():
    from gf3_audio_modem_amd.OFDM import receiver, transmitter
    for cls in (transmitter, receiver):
        tx = cls("A2")
        assert tx.papr_reduction is False and tx.papr_target_db == 6.0 and tx.papr_iterations == 16
        assert tx.papr_tone_limit_db == 6.0 and tx.body_gain == 1.0 and tx.last_tx_report is None
    assert transmitter("A2")._check_tx() == (1.0, None) and tx_of()._check_tx() == (1.0, (6.0, 6.0, 16))


def test_facade_refusals():
    bits = np.zeros(100, dtype=np.uint8)
    for bad in (2.0, 14.0, float("nan"), float("inf"), "6", None):
        with pytest.raises(ValueError, match=r"papr target .*\[3, 13\]"):
            tx_of(papr_target_db=bad).transmit(bits)
    for bad in (-21.0, 20.5, float("nan"), None):
        with pytest.raises(ValueError, match=r"papr tone limit .*\[-20, 20\]"):
            tx_of(papr_tone_limit_db=bad).transmit(bits)
    for bad in (-1, 65, 16.0, "16", None, True):
        with pytest.raises(ValueError, match=r"papr iterations .*\[0, 64\]"):
            tx_of(papr_iterations=bad).transmit(bits)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="body_gain must be a finite number > 0"):
            tx_of(body_gain=bad).transmit(bits)
        with pytest.raises(ValueError, match="body_gain must be a finite number > 0"):
            tx_of(body_gain=bad, papr_reduction=False).transmit(bits)
    for mode in ("A1", "B1", "C1"):
        with pytest.raises(ValueError, match=r"at least 8 reserved carriers.*leaves 1 .*\*1 modes"):
            tx_of(mode).transmit(bits)
    with pytest.raises(NotImplementedError, match="papr_reduction with bit_loading"):
        tx_of(bit_loading=np.full(1400, 2, dtype=np.uint8)).transmit(bits)


def test_tx_report_keys_and_values():
    """`_tx_report` on rows built by hand: N = 4096, CP = 224, P = 2, D = 4, two packets."""
    tx = tx_of()
    S, Lc, M = 4096 + 224, tx.chirp_length, 2 * 2 + 4
    rows = np.zeros((2, Lc + M * S))
    rows[:, :Lc] = 0.2 * np.cos(np.arange(Lc))
    rows[0, 7] = -0.2
    body = rows[:, Lc:].reshape(2, M, S)
    body[:] = 0.01
    body[1, 0, 5] = -0.11                                                # a pilot sample
    body[0, 3, 300] = 0.08                                               # a data sample
    body[1, 4, 3] = 0.5                                                  # inside a data symbol's prefix: not judged
    plain = tx._tx_report(rows)
    assert set(plain) == {"chirp_peak", "pilot_peak", "data_peak", "body_rms", "papr_db", "headroom_db"}
    assert plain["chirp_peak"] == 0.2 and plain["pilot_peak"] == 0.11 and plain["data_peak"] == 0.08
    assert plain["body_rms"] == pytest.approx(np.sqrt(np.mean(body ** 2)), rel=1e-14)
    assert plain["headroom_db"] == pytest.approx(20 * np.log10(0.2 / 0.11), rel=1e-12)
    sym = body[0, 3, 224:]
    assert plain["papr_db"] == pytest.approx(20 * np.log10(0.08 / np.sqrt(np.mean(sym ** 2))), rel=1e-12)
    found = np.zeros((2, 4, 4))
    found[..., 0], found[..., 2] = 0.03, 5.0
    found[1, 2, 0], found[0, 0, 2] = 0.05, 13.0
    under = tx._tx_report(rows, found, gain=1.5)
    assert set(under) == set(plain) | {"data_peak_zero_filler", "best_index_mean"}
    assert under["data_peak_zero_filler"] == pytest.approx(2 * 1.5 * 0.05, rel=1e-15) and under["best_index_mean"] == 6.0
    assert {k: under[k] for k in plain} == plain
