"""Impulse blanking ahead of the demodulator, host side (no GPU): the NumPy restatement (tests/blank_ref.py) pinned on
hand-made bodies, the declared ABI and the façade's defaults, and what blanking buys on a packet under frequent clicks with
the oracle's demodulation, the restated carrier x symbol weights and the restated decoder."""
import os
import re

import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import blank_ref as BR
from tests import impulse_ref as IR
from tests import ldpc_ref as R
from tests.util import modeA2_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0])


def hand_made():
    """3 samples | a body of M = 5 symbols of S = 8 samples | 3 samples.  Baseline 10.  Symbol 1 is the quietest (energy
    0.25), symbol 2 the second quietest (+-1 around 10: energy exactly 1), so rank (5 - 1) // 4 = 1 picks symbol 2:
    mu = 10, sigma = 1, and kappa = 3 gives T = 3.  Planted: 19 on the body's first sample, 13 (|v - mu| = T exactly: the
    compare is strict, not flagged) on sample 4, 1 on the last sample of symbol 3 (body sample 31), 19 on the body's last
    sample (39).  The samples around the body are 100."""
    body = np.concatenate([10 + PATTERN, 10 + 0.5 * PATTERN, 10 + PATTERN, 10 + PATTERN, 10 + PATTERN])
    body[0], body[4], body[31], body[39] = 19.0, 13.0, 1.0, 19.0
    return np.concatenate([np.full(3, 100.0), body, np.full(3, 100.0)])


@pytest.mark.parametrize("guard,blanked,counts", [
    (0, [0, 31, 39], [1, 0, 0, 1, 1]),
    (1, [0, 1, 30, 31, 32, 38, 39], [2, 0, 0, 2, 3]),
    (2, [0, 1, 2, 29, 30, 31, 32, 33, 37, 38, 39], [3, 0, 0, 3, 5])])
def test_hand_made_body(guard, blanked, counts):
    x = hand_made()
    out, cnt, level, energy, det = BR.blank(x, [3], 5, 8, kappa=3.0, guard=guard, details=True)
    assert level.tolist() == [[10.0, 1.0]]
    assert energy[0, 1] == 0.25 and energy[0, 2] == 1.0 and (energy[0, [0, 3, 4]] > 1.0).all()
    assert np.flatnonzero(det["flags"][0]).tolist() == [0, 31, 39]
    assert np.flatnonzero(det["blanked"][0]).tolist() == blanked
    assert cnt.dtype == np.int32 and cnt.tolist() == [counts]
    want = x.copy()
    want[3 + np.array(blanked)] = 10.0
    assert np.array_equal(out, want)
    assert (out[:3] == 100).all() and (out[-3:] == 100).all()          # the guard never leaves the body
    assert np.array_equal(x, hand_made())                              # (the input is not written)
    # a caller's pattern in the second buffer stays everywhere but at the blanked samples
    filled = BR.blank(x, [3], 5, 8, kappa=3.0, guard=guard, out=np.full(len(x), -7.0))[0]
    assert np.array_equal(np.flatnonzero(filled != -7.0), 3 + np.array(blanked)) and (filled[3 + np.array(blanked)] == 10).all()


def test_rank_rule_and_its_tie_rule():
    assert [BR.rank_of(M) for M in (1, 2, 4, 5, 8, 9)] == [0, 0, 0, 1, 1, 2]
    for M in (1, 2, 4, 5, 8, 9):
        e = np.random.default_rng(M).permutation(M).astype(float)      # energy = its own rank
        assert e[BR.pick(e)] == BR.rank_of(M)
    assert BR.pick([2.0, 1.0, 1.0, 1.0, 3.0]) == 2                      # order 1, 2, 3, 0, 4: rank 1 is index 2
    assert BR.pick([1.0, 1.0]) == 0 and BR.pick([5.0, 5.0, 5.0, 5.0, 5.0]) == 1
    assert BR.pick([np.inf, 3.0, np.inf, 2.0, 1.0, np.inf, np.inf, np.inf, np.inf]) == 1     # rank 2 of 1, 2, 3, inf, ...


def test_integer_storage_rounds_the_baseline_half_to_even():
    # u8 around 128 with a click: replaced by 128
    x = np.tile(np.array([127, 129], dtype=np.uint8), 20)
    x[13] = 255
    out, cnt, level, _ = BR.blank(x, [0], 5, 8, kappa=4.5, guard=0)
    assert out.dtype == np.uint8 and level.tolist() == [[128.0, 1.0]] and cnt.sum() == 1 and out[13] == 128
    assert np.array_equal(np.delete(out, 13), np.delete(x, 13))
    # 127.5 and 128.5 both round to 128; 126.5 rounds to 126
    for lo, want in ((127, 128), (128, 128), (126, 126)):
        x = np.tile(np.array([lo, lo + 1], dtype=np.uint8), 20)
        x[13] = 0
        out, _, level, _ = BR.blank(x, [0], 5, 8, kappa=4.5, guard=0)
        assert level[0, 0] == lo + 0.5 and out[13] == want
    # i16 with a baseline away from zero, and the clamp of a baseline beyond the type (cannot arise from i16 samples: by hand)
    x = np.tile(np.array([-3001, -2999], dtype=np.int16), 20)
    x[7] = 32767
    out, _, level, _ = BR.blank(x, [0], 5, 8)
    assert level[0, 0] == -3000 and out[7] == -3000 and out.dtype == np.int16
    assert BR.to_storage(1e9, np.int16) == 32767 and BR.to_storage(-1e9, np.int16) == -32768 and BR.to_storage(300.0, np.uint8) == 255
    assert BR.to_storage(0.1, np.float32) == np.float32(0.1)


def test_non_finite_samples_are_blanked_and_left_out_of_the_sums():
    x = np.concatenate([10 + 0.5 * PATTERN, np.tile(10 + PATTERN, 3), 10 + 0.5 * PATTERN])
    x[9], x[18], x[27] = np.nan, np.inf, -np.inf
    want = x.copy()
    want[[9, 18, 27]] = 10.0
    out, cnt, level, energy = BR.blank(x, [0], 5, 8, kappa=4.5, guard=0)
    assert cnt.tolist() == [[0, 1, 1, 1, 0]] and np.array_equal(out, want)
    assert np.isfinite(energy).all() and energy[0, 0] == 0.25 and level.tolist() == [[10.0, 0.5]]
    # seven samples of symbol 1 are left, four at 11 and three at 9: mean 10 + 1/7 and energy 48/49, not NaN
    assert energy[0, 1] == pytest.approx(1.0 - 1.0 / 49.0, rel=1e-12)
    # a symbol without a finite sample: energy +Inf, it sorts last and is blanked whole
    x = np.tile(10 + PATTERN, 5)
    x[8:16] = np.nan
    out, cnt, level, energy = BR.blank(x, [0], 5, 8, guard=0)
    assert energy[0, 1] == np.inf and np.argsort(energy[0], kind="stable")[-1] == 1
    assert cnt.tolist() == [[0, 8, 0, 0, 0]] and level.tolist() == [[10.0, 1.0]] and (out[8:16] == 10).all()


def test_threshold_zero_and_infinite():
    # a silent body: sigma = 0, T = 0 flags whatever differs from mu
    x = np.full(46, 3.0)
    x[20] = 3.0000001
    x[1] = 9.0                                                         # (outside the body)
    out, cnt, level, _ = BR.blank(x, [3], 5, 8, kappa=4.5, guard=1)
    assert level.tolist() == [[3.0, 0.0]] and cnt.tolist() == [[0, 0, 3, 0, 0]] and out[1] == 9.0 and out[20] == 3.0
    # more than three quarters of the symbols without a finite sample: the ranked symbol has energy +Inf and mean 0, so
    # T = Inf flags the non-finite samples only, and they become 0
    x = np.full(40, np.nan)
    x[8:16] = 10 + 100 * PATTERN
    out, cnt, level, energy = BR.blank(x, [0], 5, 8, guard=0)
    assert level.tolist() == [[0.0, np.inf]] and cnt.tolist() == [[8, 0, 8, 8, 8]]
    assert np.array_equal(out[8:16], x[8:16]) and not out[:8].any() and not out[16:].any()


def test_ragged_packet_writes_nothing():
    x = np.tile(10 + PATTERN, 6)
    x[[2, 12, 45]] = 50.0
    out, cnt, level, energy = BR.blank(x, [-1, 4, 9], 5, 8, guard=0)
    assert cnt[0].tolist() == [-1] * 5 and cnt[2].tolist() == [-1] * 5 and (cnt[1] >= 0).all() and cnt[1].sum() == 1
    assert not energy[[0, 2]].any() and not level[[0, 2]].any() and level[1, 1] > 0
    assert out[12] == level[1, 0] and out[2] == 50.0 and out[45] == 50.0       # 2: before body 1; 45: behind it
    out, cnt, _, _ = BR.blank(x, [8], 5, 8)                             # [8, 48) fits exactly
    assert (cnt >= 0).all()
    assert (BR.blank(x, [9], 5, 8)[1] == -1).all()


def test_abi_name_is_declared_and_bound():
    from gf3_audio_modem_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gf3rx.h")).read()
    assert "gf3_blank_impulses" in set(re.findall(r"\b(gf3_[a-z_]+)\s*\(", hdr))
    res, args = _lib._SIGS["gf3_blank_impulses"]
    assert len(args) == 12
    unit = os.path.join(ROOT, "gf3_audio_modem_amd", "csrc", "gf3rx_blank.hip")
    from gf3_audio_modem_amd import build
    assert unit in build.SRC and "gf3_blank_impulses" in open(unit).read()


def test_facade_defaults_and_refusals_before_any_gpu_work():
    from gf3_audio_modem_amd.engine import Engine
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2", encoding="XOR")
    assert rx.impulse_blanking is False and rx.blanking_threshold == 4.5 and rx.blanking_guard == 8
    assert rx.last_blanked is None and rx.last_sample_level is None
    assert Engine.check_blanking(4.5, 8) == (4.5, 8) and Engine.check_blanking(1, np.int64(64)) == (1.0, 64)
    for bad in (0.0, -1.0, np.nan, np.inf, "x", None):
        with pytest.raises(ValueError, match="threshold"):
            Engine.check_blanking(bad, 8)
    for bad in (-1, 65, 8.0, None, True):
        with pytest.raises(ValueError, match="guard"):
            Engine.check_blanking(4.5, bad)
    rx.impulse_blanking = True
    rx.blanking_guard = 65
    with pytest.raises(ValueError, match="guard"):                      # (no engine exists yet: nothing touched the GPU)
        rx.receive(np.zeros(10))
    rx.blanking_guard, rx.blanking_threshold = 8, 0.0
    with pytest.raises(ValueError, match="threshold"):
        rx.receive(np.zeros(10))
    assert not rx._engines


# ---- a packet under frequent clicks ---------------------------------------------------------------------------------
D, C, P, S, M = 180, 1400, 20, 4320, 220


def click_failures(p, sig, start, cw, msg, sh, share, amplitude, seed=11):
    """White noise 15 dB below the body plus the click scenario, then the oracle's demodulation, the restated carrier x
    symbol weights, the de-interleaver and the restated decoder at 20 iterations, on the samples as they are and on the
    restatement's blanked copy (kappa = 4.5, guard = 8).  -> (failed without, failed with, counts [M], level, hit, rms)"""
    rng = np.random.default_rng(seed)
    body = sig[start: start + M * S]
    rms = float(np.sqrt(np.mean(body ** 2)))
    noisy = sig + rng.normal(0.0, rms / 10 ** 0.75, sig.shape)
    clicks, hit = BR.click_scenario(sig, start, M, S, P, D, share, amplitude, rng)
    noisy = noisy + clicks
    blanked, counts, level, _ = BR.blank(noisy, [start], M, S, 4.5, 8)
    failed = []
    for r in (noisy, blanked):
        eq = orc.demod_frames(r, np.array([start]), p)["eq"]
        v_c, v_s = IR.noise_estimate2(eq, p.const_points, D)
        llr = IR.deinterleave(IR.soft_demap_nw2(eq, v_c, v_s, p.const_points, p.const_bits), D, C, 2)
        bits, _, it = R.decode(sh, llr[: cw.size].reshape(cw.shape), 20)
        failed.append(int(np.sum((bits != msg).any(axis=1) | (it < 0))))
    return failed[0], failed[1], counts[0], level[0], hit, float(np.sqrt(np.mean((noisy - clicks)[start: start + M * S] ** 2)))


def test_blanking_decodes_a_packet_under_frequent_clicks():
    """Mode A2, QPSK, one packet of 328 interleaved rate-1/2 codewords from the oracle's synthesiser (seed 7), white noise
    15 dB below the signal and a 200-sample burst of white noise at `amplitude` x the body's rms at a random place in
    `share` of the data symbols and in start pilots 3 and 11 (seed 11).  Failed codewords of 328, without | with blanking:
    share 0.6 at x16, x20, x24: 328 | 0 each;  share 0.3 at x20: 0 | 0 (the symbol weights alone still cope).  Hit symbols
    had 211 to 233 samples blanked; the 110 clean symbols of the share-0.6 rows 34 in all, 17 at most in one (the tail of
    the previous symbol's burst and guard); the level read 0.999 x the rms of the noisy body without its clicks."""
    from gf3_audio_modem_amd.ldpc import shift_table
    sh = shift_table("1/2")
    rng = np.random.default_rng(7)
    p = modeA2_params(rng.integers(0, 2, size=4094).astype(np.uint8))
    n_cw = D * C * 2 // 1536
    msg = rng.integers(0, 2, size=(n_cw, 768), dtype=np.uint8)
    cw = R.encode(sh, msg)
    bits = rng.integers(0, 2, size=D * C * 2, dtype=np.uint8)
    bits[: cw.size] = cw.reshape(-1)
    fill = orc.qpsk_table()[0][rng.integers(0, 4, size=p.K - p.C)]
    sig = orc.tx_stream(IR.interleave(bits, D, C, 2), fill, p, lead=2000, tail=2000)
    sig = sig[: 2000 + p.frame_len + 2000]                  # (the terminating chirp is not needed: the start is given)
    start = 2000 + p.Lc
    for share, amplitude in ((0.6, 16.0), (0.6, 20.0), (0.6, 24.0), (0.3, 20.0)):
        without, with_, counts, level, hit, rms = click_failures(p, sig, start, cw, msg, sh, share, amplitude)
        clean = np.delete(counts, hit)
        print(f"share {share} x{amplitude:.0f}: failed of {n_cw} without blanking {without}, with {with_}; hit symbols hold "
              f"{counts[hit].min()}..{counts[hit].max()} blanked samples, the {len(clean)} clean ones {clean.sum()} (at most "
              f"{clean.max()}); level {level[1] / rms:.3f} x the body's rms, baseline {level[0]:.2e}")
        assert with_ == 0
        assert (without >= 300) if share == 0.6 else (without == 0)
