"""Per-symbol phase and timing tracking, host side (no GPU): the NumPy restatement (tests/track_ref.py) on planted
tracks, its coasting rules, and the decoding gain on a packet whose delay wanders between the pilots, with the oracle's
demodulation and the restated decoder (tests/ldpc_ref.py)."""
import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import ldpc_ref as R
from tests import noise_ref as NR
from tests import track_ref as TR
from tests.util import modeA2_params

PTS, BITS = orc.qpsk_table()
D, C = 180, 1400
BINS = np.arange(100, 1500)                                # mode A2
KAP = TR.kappa(BINS)
KMAX = np.abs(KAP).max()


def planted(points, sigma, seed, peak_a=6.0, peak_edge=12.0, bins=BINS, D=D):
    """Random points of the table, rotated by exp(i (a_l + b_l kappa_c)) with a_l, b_l max|kappa| swinging to peak_a and
    peak_edge rad in mid-packet, plus noise of `sigma` per component.  -> (eq [D, C], a [D], b [D])"""
    rng = np.random.default_rng(seed)
    kap = TR.kappa(bins)
    a, b = TR.swing(D, peak_a), TR.swing(D, peak_edge) / np.abs(kap).max()
    idx = rng.integers(0, len(points), size=(D, len(kap)))
    eq = points[idx] * np.exp(1j * (a[:, None] + b[:, None] * kap))
    return eq + (rng.normal(size=eq.shape) + 1j * rng.normal(size=eq.shape)) * sigma, a, b


def edge_error(phase, a, b, kmax=KMAX):
    """|a^ - a| + |b^ - b| max|kappa| per symbol: the phase error of the worst carrier, in rad."""
    return np.abs(phase[..., 0] - a) + np.abs(phase[..., 1] - b) * kmax


def noise_bound(sigma, es, n_sigma=6.0):
    """n_sigma standard deviations of the two estimates' noise at the band edge, when every decision is right: the
    common phase has variance sigma^2 / (C Es), the slope sigma^2 / (Es sum kappa^2)."""
    return n_sigma * sigma / np.sqrt(es) * (1 / np.sqrt(C) + KMAX / np.sqrt((KAP ** 2).sum()))


def test_follows_a_planted_swing_and_slips_without_the_velocity_term():
    """QPSK, sigma 0.35 per component (2.2 % of the decisions wrong on a static stream), 6 rad common and 12 rad at the
    band edge: the steepest step is 18 pi / 180 = 0.31 rad per symbol at the band edge, inside QPSK's pi / 4 on its own but
    not with this noise on top, while the step's own change, 18 * 2 pi^2 / 180^2 = 0.011 rad per symbol, is nothing."""
    eq, a, b = planted(PTS, 0.35, seed=1)
    _, phase, measured = TR.track(eq, PTS, BINS, D)
    err = edge_error(phase[0], a, b)
    print(f"QPSK: band-edge error max {err.max():.4f} rad, bound {noise_bound(0.35, 1.0):.4f}; end of track {phase[0, -1]}")
    assert measured.all() and err.max() < noise_bound(0.35, 1.0)
    assert edge_error(phase[0, -1:], 0.0, 0.0)[0] < 0.05 + noise_bound(0.35, 1.0)       # (the swing's last half step)
    _, slow, _ = TR.track(eq, PTS, BINS, D, velocity=False)
    e0 = edge_error(slow[0], a, b)
    print(f"without velocity: band-edge error max {e0.max():.3f} rad, at the end {e0[-1]:.3f}")
    assert e0.max() > np.pi / 4                            # past the decision boundary: a slip


def test_follows_on_16qam():
    pts, _ = orc.square_qam_table(4)
    eq, a, b = planted(pts, 0.12, seed=2)
    _, phase, measured = TR.track(eq, pts, BINS, D)
    err = edge_error(phase[0], a, b)
    print(f"16-QAM: band-edge error max {err.max():.4f} rad, bound {noise_bound(0.12, 1.0):.4f}")
    assert measured.all() and err.max() < noise_bound(0.12, 1.0)


def test_coasts_through_clicks_and_resumes():
    eq, a, b = planted(PTS, 0.35, seed=3)
    rng = np.random.default_rng(30)
    hit = [60, 61, 62]                                     # in mid-swing: the track moves 0.2 rad per symbol there
    eq[hit] += (rng.normal(size=(3, C)) + 1j * rng.normal(size=(3, C))) * 5.0
    _, phase, measured = TR.track(eq, PTS, BINS, D)
    want = np.ones(D, dtype=np.uint8)
    want[hit] = 0
    assert np.array_equal(measured[0], want)
    err = edge_error(phase[0], a, b)
    print(f"clicks: band-edge error in the gap {err[hit]}, after it max {err[63:].max():.4f}")
    # in the gap the velocity carries on; what it misses is the swing's curvature, 0.011 rad per symbol squared: 1, 3, 6 steps
    assert (err[hit] < 6 * 0.011 + 2 * noise_bound(0.35, 1.0)).all()
    assert err[63:].max() < noise_bound(0.35, 1.0)


def test_zero_inf_and_nan_inputs():
    eq, a, b = planted(PTS, 0.1, seed=4)
    eq[40] = 0.0                                           # an all-zero row: den = 0
    eq[90] = complex(np.inf, 0.0)                          # a row of Inf: nothing enters the sums
    eq[120, 7] = complex(np.nan, 1.0)                      # single carriers: only left out
    eq[121, 1399] = complex(0.2, -np.inf)
    out, phase, measured, det = TR.track(eq, PTS, BINS, D, details=True)
    want = np.ones(D, dtype=np.uint8)
    want[[40, 90]] = 0
    assert np.array_equal(measured[0], want)
    assert det["den"][0, 40] == 0.0 and det["den"][0, 90] == 0.0 and det["finite"].all()
    for l in (40, 90):                                     # coasting: the velocity of the symbol before carries on
        np.testing.assert_allclose(phase[0, l], 2 * phase[0, l - 1] - phase[0, l - 2], rtol=0, atol=1e-12)
    assert edge_error(phase[0], a, b).max() < noise_bound(0.1, 1.0) + 2 * 0.011
    fin = np.isfinite(out.real) & np.isfinite(out.imag)
    assert np.array_equal(fin, np.isfinite(eq.real) & np.isfinite(eq.imag)) and (~fin).sum() == C + 2
    assert not out[40].any()


def test_a_single_carrier_always_coasts():
    rng = np.random.default_rng(5)
    eq = PTS[rng.integers(0, 4, size=(2 * 7, 1))] * np.exp(0.3j)
    out, phase, measured = TR.track(eq, PTS, [812], 7)
    assert not measured.any() and not phase.any() and measured.shape == (2, 7) and phase.shape == (2, 7, 2)
    assert np.array_equal(out, eq)


def test_kappa_comes_from_the_bins_not_from_the_column():
    """A permuted carrier list with its columns permuted alike gives the same track and the permuted output."""
    rng = np.random.default_rng(6)
    bins = np.arange(5, 400, 3)                            # a comb
    eq, a, b = planted(PTS, 0.1, seed=6, peak_a=2.0, peak_edge=4.0, bins=bins, D=20)
    out, phase, _ = TR.track(eq, PTS, bins, 20)
    perm = rng.permutation(len(bins))
    out_p, phase_p, _ = TR.track(eq[:, perm], PTS, bins[perm], 20)
    np.testing.assert_allclose(phase_p, phase, rtol=0, atol=1e-12)
    np.testing.assert_allclose(out_p, out[:, perm], rtol=0, atol=1e-12)
    assert edge_error(phase[0], a, b, np.abs(TR.kappa(bins)).max()).max() < 0.05


# ---- a packet whose delay wanders between the pilots ---------------------------------------------------------------
def wander_failures(p, sig, first, cw, msg, sh, tau0, seed=7):
    """Failed codewords without and with the tracker on the stream delayed by tau0 and with white noise 12 dB below the
    signal: the oracle's demodulation, noise weights and the restated decoder (20 iterations).  -> (without, with, phase)"""
    rng = np.random.default_rng(seed)
    noisy = TR.delay_wander(sig, first, p.S, p.D, tau0)
    noisy = noisy + rng.normal(0, np.sqrt(np.mean(sig ** 2) / 10 ** 1.2), sig.shape)
    eq = orc.demod_frames(noisy, np.array([first - p.P * p.S]), p)["eq"]
    tracked, phase, measured = TR.track(eq, p.const_points, p.data_carriers, p.D)
    failed = []
    for e in (eq, tracked):
        llr = NR.soft_demap_nw(e, NR.noise_estimate(e, p.const_points, p.D), p.const_points, p.const_bits, p.D)
        bits, _, it = R.decode(sh, llr[: cw.size].reshape(cw.shape), 20)
        failed.append(int(np.sum((bits != msg).any(axis=1) | (it < 0))))
    return failed[0], failed[1], phase, measured


def test_tracker_decodes_a_packet_whose_delay_wanders():
    """Mode A2, QPSK, one packet of 328 rate-1/2 codewords in stream order from the oracle's synthesiser, white noise 12 dB
    below the signal, every data symbol delayed by tau0 sin^2(pi (l + 1/2) / D) samples: the pilots at both ends see none of
    it.  Failed codewords of 328, without | with the tracker, seed 7:  tau0 = 0: 0 | 0,  1.2: 180 | 0,  1.5: 202 | 0,
    1.8: 214 | 0."""
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
    sig = orc.tx_stream(bits, fill, p, lead=2000, tail=2000)
    sig = sig[: 2000 + p.frame_len + 2000]                  # (the terminating chirp is not needed: the start is given)
    first = 2000 + p.Lc + p.P * p.S
    for tau0 in (0.0, 1.2, 1.5, 1.8):
        without, tracked, phase, measured = wander_failures(p, sig, first, cw, msg, sh, tau0)
        slope = 2 * np.pi * tau0 / p.N
        print(f"tau0 {tau0}: failed codewords without {without}, with the tracker {tracked}; slope peak "
              f"{np.abs(phase[0, :, 1]).max():.3e} planted {slope:.3e}; end of track {phase[0, -1]}")
        assert tracked == 0 and measured.all()
        assert (without == 0) if tau0 == 0 else (without > 0)
        if tau0:
            assert abs(np.abs(phase[0, :, 1]).max() / slope - 1) < 0.2
