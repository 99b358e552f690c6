"""Per-symbol phase and timing tracking on the GPU: gf3_track_phase against the NumPy restatement (tests/track_ref.py) on
the smallest shapes at which the kernel can go wrong, its coasting rules and refusals, and `phase_tracking` end to end
through the façade on a packet whose delay wanders between the pilots.

Tolerance of the comparison.  The two sides add the same C terms per sum in different orders, each with a relative error of
at most C 2^-53 of the sum of the terms' magnitudes: e1 = C 2^-52 between them.  A measurement moves the band-edge phase
|a| + |b| max|kappa| by at most e1 rho (1 + 3): rho = sum |r| / |S0| < 1.25 at the noise levels used here, 1 for the common
phase and max|kappa| sum |kappa r| / sum kappa^2 |r| <= 3 for the slope on a band that is uniformly filled (a comb and a
permutation of it are).  A measured symbol forgets the error of its prediction (da is measured against it), so errors do
not add up along a packet, except through coasting: n coasting symbols carry the velocity's error, twice a measurement's,
n times on: (1 + 2 n) = 7 for the three in a row at most that are planted here.  5 x 7 = 35; the factor is 64, and C counts
as 64 at least, which leaves the few-ulp errors of sincos and atan2 (they do not grow with C) 4096 ulps of room.
64 x 2047 x 2^-52 = 2.9e-11 at the largest C: below 1e-9."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import ldpc_ref as R
from tests import noise_ref as NR
from tests import track_ref as TR
from tests.util import modeA2_params

pytestmark = pytest.mark.gpu
QPSK = orc.qpsk_table()
RING8 = (np.exp(2j * np.pi * (np.arange(8) + 0.25) / 8) * (1.0 + 0.3 * (np.arange(8) % 2)),
         (np.arange(8)[:, None] >> np.arange(2, -1, -1)) & 1)
PARITY = {}


def tolerance(C):
    return 64.0 * max(C, 64) * 2.0 ** -52


def engine_of(bins, table=QPSK, D=7, N=4096):
    from gf3_audio_modem_amd import Engine, RxConfig
    pts, bits = table
    mu = np.asarray(bits).shape[1]
    return Engine(RxConfig(N=N, CP=0, P=1, D=D, data_bins=np.asarray(bins), const_points=np.asarray(pts),
                           const_bits=np.asarray(bits).astype(np.int64), known_bits=np.zeros((N // 2 - 1) * mu, np.uint8),
                           in_dtype=torch.float64, fit_lo=10, fit_hi=100))


def ramps(F, D, steps):
    """Per packet a track that grows linearly: a = step (l + 1) / 2, b max|kappa| = step (l + 1)."""
    l1 = np.arange(1, D + 1)
    s = np.asarray([steps[f % len(steps)] for f in range(F)])[:, None]
    return 0.5 * s * l1, s * l1


def synth(pts, bins, F, D, sigma, steps, seed):
    """Random points of the table under the planted ramps plus noise of `sigma` per component -> eq [F*D, C]"""
    rng = np.random.default_rng(seed)
    kap = TR.kappa(bins)
    kmax = np.abs(kap).max() or 1.0
    a, e = ramps(F, D, steps)
    idx = rng.integers(0, len(pts), size=(F, D, len(kap)))
    eq = np.asarray(pts)[idx] * np.exp(1j * (a[..., None] + (e / kmax)[..., None] * kap))
    eq = eq + (rng.normal(size=eq.shape) + 1j * rng.normal(size=eq.shape)) * sigma
    return eq.reshape(F * D, len(kap))


def record(case, ratio):
    PARITY[case] = float(ratio)
    path = os.environ.get("GF3_TRACK_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            json.dump({"largest error / tolerance per case": PARITY, "tolerance": "64 max(C, 64) 2^-52"}, fh, indent=1)
            fh.write("\n")


def compare(case, eng, eq, pts, bins, D, coasting=()):
    """The precondition on the inputs (asserted on the restatement), then kernel == restatement: `measured` equal, the track
    to the tolerance in band-edge radians, `out` to the tolerance x max|eq| with the same non-finite positions."""
    eq = np.asarray(eq, dtype=np.complex128)
    C = eq.shape[1]
    F = eq.shape[0] // D
    ref_out, ref_phase, ref_meas, det = TR.track(eq, pts, bins, D, details=True)
    sure_meas, sure_coast = TR.robust(det)
    planted = np.zeros((F, D), dtype=bool)
    for f, l in coasting:
        planted[f, l] = True
    # (planted coasting symbols apart: an all-zero row ties every QPSK point exactly, on both sides alike, and its sums do
    # not depend on the pick -- r = 0, |s| the same; no decision of a coasting symbol reaches the track or `out`)
    assert det["margin"][~planted].min(initial=np.inf) > 1e-9, f"{case}: a decision of the restatement is a near tie"
    assert np.array_equal(sure_coast, planted) and np.array_equal(sure_meas, ~planted), f"{case}: a gate without margin"
    assert np.array_equal(ref_meas != 0, ~planted)
    out, phase, measured = eng.track_phase(eq, want_track=True)
    assert out.dtype == torch.complex128 and tuple(out.shape) == (F * D, C)
    assert phase.dtype == torch.float64 and tuple(phase.shape) == (F, D, 2)
    assert measured.dtype == torch.uint8 and tuple(measured.shape) == (F, D)
    out, phase, measured = out.cpu().numpy(), phase.cpu().numpy(), measured.cpu().numpy()
    assert np.array_equal(measured, ref_meas)
    kmax = np.abs(TR.kappa(bins)).max()
    d = phase - ref_phase
    e_phase = (np.abs(d[..., 0]) + np.abs(d[..., 1]) * kmax).max() if d.size else 0.0
    fin = np.isfinite(eq.real) & np.isfinite(eq.imag)
    assert np.array_equal(np.isfinite(out.real) & np.isfinite(out.imag), fin)
    assert np.array_equal(np.isfinite(ref_out.real) & np.isfinite(ref_out.imag), fin)
    e_out = np.abs(out[fin] - ref_out[fin]).max() / np.abs(eq[fin]).max() if fin.any() else 0.0
    tol = tolerance(C)
    print(f"{case}: C {C} D {D} F {F}: track error {e_phase:.3e} rad, out error {e_out:.3e} of max|eq|, tolerance {tol:.3e}")
    record(case, max(e_phase, e_out) / tol)
    assert e_phase <= tol and e_out <= tol
    return out, phase, measured


# ---- shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,N", [(1, 4096), (2, 4096), (63, 4096), (65, 4096), (513, 4096), (1025, 4096), (1537, 4096),
                                 (2047, 4096), (2049, 8192)])
def test_carrier_counts(C, N):
    """One wave's worth and less, one carrier past each carriers-per-thread step of the 512-thread workgroup (512, 1024,
    1536, 2048), every carrier of N = 4096.  Packet 0 ends on a large phase, packet 1 has none: state that leaked
    across packets would start packet 1 at packet 0's phase and velocity."""
    bins = np.arange(N // 2 - 1 - C, N // 2 - 1) + 1
    D, F = 7, 3
    eq = synth(QPSK[0], bins, F, D, 0.1, (0.3, 0.0, -0.15), seed=C)
    coasting = [(f, l) for f in range(F) for l in range(D)] if C == 1 else ()       # kappa = 0: den = 0, always
    out, phase, _ = compare(f"carriers_{C}", engine_of(bins, N=N), eq, QPSK[0], bins, D, coasting)
    kmax = np.abs(TR.kappa(bins)).max()
    if C > 1:
        assert abs(phase[0, -1, 1]) * kmax > 1.5                   # planted: 2.1 rad at the band edge
    if C >= 63:                                                    # (6 sigma of the noise of C = 63 carriers)
        assert (np.abs(phase[1, :, 0]) + np.abs(phase[1, :, 1]) * kmax).max() < 0.2
    if C == 1:
        assert np.array_equal(out, eq) and not phase.any()


@pytest.mark.parametrize("D,F", [(1, 1), (1, 3), (2, 1), (2, 3), (7, 1)])
def test_symbols_and_packets(D, F):
    bins = np.arange(300, 365)
    eq = synth(QPSK[0], bins, F, D, 0.1, (0.3, 0.0, -0.15), seed=10 * D + F)
    compare(f"D{D}_F{F}", engine_of(bins, D=D), eq, QPSK[0], bins, D)


@pytest.mark.parametrize("kind", ["comb", "permuted"])
def test_carrier_maps(kind):
    """kappa comes from the bins: a comb (every third bin) and the same comb listed in a random order."""
    bins = np.arange(7, 7 + 3 * 600, 3)
    if kind == "permuted":
        bins = np.random.default_rng(8).permutation(bins)
    eq = synth(QPSK[0], bins, 2, 7, 0.1, (0.3, -0.2), seed=len(kind))
    _, phase, _ = compare(kind, engine_of(bins), eq, QPSK[0], bins, 7)
    a, e = ramps(2, 7, (0.3, -0.2))
    kmax = np.abs(TR.kappa(bins)).max()
    assert np.abs(phase[..., 0] - a).max() < 0.05 and np.abs(phase[..., 1] * kmax - e).max() < 0.05


@pytest.mark.parametrize("kind", ["qam4_binary", "qam16", "qam64", "ring8"])
def test_tables(kind):
    """The straight-line grid kernels (2, 4 and 8 levels per axis) and, for a table that is no grid, the literal scan (which the
    reference's QPSK table, whose first label bit belongs to the Q axis, takes in every other test here)."""
    table, sigma, step = {"qam4_binary": (orc.square_qam_table(2), 0.1, 0.3), "qam16": (orc.square_qam_table(4), 0.03, 0.1),
                          "qam64": (orc.square_qam_table(6), 0.015, 0.03), "ring8": (RING8, 0.06, 0.15)}[kind]
    bins = np.arange(5, 400)
    eq = synth(table[0], bins, 2, 7, sigma, (step, -step / 2), seed=len(kind))
    compare(kind, engine_of(bins, table), eq, table[0], bins, 7)


GRID_TABLES = {"qam4_binary": (2, 0.1, 0.3), "qam16": (4, 0.03, 0.1), "qam64": (6, 0.015, 0.03)}


def grid_case(kind, C, N):
    """-> (table, bins, eq): F = 2, D = 3, the top C bins, the noise and the ramps of test_tables."""
    mu, sigma, step = GRID_TABLES[kind]
    table = orc.square_qam_table(mu)
    bins = np.arange(N // 2 - 1 - C, N // 2 - 1) + 1
    return table, bins, synth(table[0], bins, 2, 3, sigma, (step, -step / 2), seed=C + mu)


@pytest.mark.parametrize("C,N", [(513, 4096), (1025, 4096), (1537, 4096), (2049, 8192)])
@pytest.mark.parametrize("kind", list(GRID_TABLES))
def test_grid_tables_at_every_carriers_per_thread_step(kind, C, N):
    """track_phase_kernel<HI, CPT> for HI = 1, 2, 3 at CPT = 2, 3, 4 and 8: test_tables runs the grid kernels at one carrier
    per thread only, test_carrier_counts walks the steps with the reference's QPSK (HI = 0)."""
    table, bins, eq = grid_case(kind, C, N)
    compare(f"{kind}_{C}", engine_of(bins, table, D=3, N=N), eq, table[0], bins, 3)


# ---- coasting -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [65, 1025])
def test_coasting_symbols_and_left_out_carriers(C):
    """Packet 0: symbol 2 under sigma = 5 noise (E > P), symbol 4 all zero (den = 0), symbol 5 all Inf (nothing enters the
    sums): they coast on the velocity and the track resumes; NaN / Inf carriers in symbols 1 and 6 are only left out.
    Packet 1: three clicked symbols in a row."""
    bins = np.arange(200, 200 + C)
    D, F = 7, 2
    eq = synth(QPSK[0], bins, F, D, 0.1, (0.3, -0.2), seed=C + 1)
    rng = np.random.default_rng(C)
    click = lambda n: (rng.normal(size=(n, C)) + 1j * rng.normal(size=(n, C))) * 5.0
    eq[2] += click(1)[0]
    eq[4] = 0.0
    eq[5] = complex(np.inf, -np.inf)
    eq[1, 3] = complex(np.nan, 0.2)
    eq[6, C - 1] = complex(0.1, np.inf)
    eq[6, 0] = complex(np.nan, np.nan)
    eq[D + 2: D + 5] += click(3)
    coasting = [(0, 2), (0, 4), (0, 5), (1, 2), (1, 3), (1, 4)]
    out, phase, measured = compare(f"coasting_{C}", engine_of(bins), eq, QPSK[0], bins, D, coasting)
    assert measured.tolist() == [[1, 1, 0, 1, 0, 0, 1], [1, 1, 0, 0, 0, 1, 1]]
    assert not out[4].any() and not np.isfinite(out[5].real).any() and np.isfinite(out[6, 1:C - 1].real).all()
    a, e = ramps(F, D, (0.3, -0.2))
    kmax = np.abs(TR.kappa(bins)).max()
    # the track has resumed: the last symbols are within 4 sigma of the noise of C = 65 carriers, 0.1 (1 + sqrt 3) / sqrt 65
    assert (np.abs(phase[:, -1, 0] - a[:, -1]) + np.abs(phase[:, -1, 1] * kmax - e[:, -1])).max() < 0.15


# ---- behaviour ------------------------------------------------------------------------------------------------------
def test_in_place_repeatable_and_without_the_track():
    bins = np.arange(100, 100 + 1400)
    D, F = 7, 3
    eng = engine_of(bins)
    eq = torch.from_numpy(synth(QPSK[0], bins, F, D, 0.1, (0.3, 0.0, -0.15), seed=77)).cuda()
    out, phase, measured = eng.track_phase(eq, want_track=True)
    again, phase2, measured2 = eng.track_phase(eq, want_track=True)
    for x, y in ((out, again), (phase, phase2), (measured, measured2)):
        assert x is not y and np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    alone = eng.track_phase(eq)
    assert isinstance(alone, torch.Tensor) and torch.equal(torch.view_as_real(alone), torch.view_as_real(out))
    work = eq.clone()
    assert eng.track_phase(work, out=work) is work                 # in place: a thread reads its elements before it writes them
    assert torch.equal(torch.view_as_real(work), torch.view_as_real(out))
    given = torch.empty(F * D * len(bins), dtype=torch.complex128, device="cuda")
    assert eng.track_phase(eq, out=given) is given and torch.equal(torch.view_as_real(given.reshape(out.shape)), torch.view_as_real(out))
    # F = 0
    o0, p0, m0 = eng.track_phase(torch.empty((0, len(bins)), dtype=torch.complex128), want_track=True)
    assert tuple(o0.shape) == (0, len(bins)) and tuple(p0.shape) == (0, D, 2) and tuple(m0.shape) == (0, D)


def test_refusals():
    from gf3_audio_modem_amd import _lib
    bins = np.arange(300, 365)
    eng = engine_of(bins)
    eq = torch.from_numpy(synth(QPSK[0], bins, 1, 7, 0.1, (0.1,), seed=3)).cuda()
    with pytest.raises(ValueError, match="eq"):
        eng.track_phase(eq[:-1])
    with pytest.raises(ValueError, match="out must be"):
        eng.track_phase(eq, out=torch.empty(eq.numel() - 1, dtype=torch.complex128, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        eng.track_phase(eq, out=torch.empty(eq.shape, dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        eng.track_phase(eq, out=torch.empty((eq.shape[0], 2 * eq.shape[1]), dtype=torch.complex128, device="cuda")[:, ::2])
    lib = _lib.load()
    out = torch.empty_like(eq)
    p, q = _lib.ptr(eq), _lib.ptr(out)
    assert lib.gf3_track_phase(eng._h, p, 0, q, None, None, None) == 0
    assert lib.gf3_track_phase(eng._h, None, 0, None, None, None, None) == 0
    for args in ((None, p, 1, q), (eng._h, None, 1, q), (eng._h, p, 1, None), (eng._h, p, -1, q)):
        assert lib.gf3_track_phase(*args, None, None, None) == _lib.GF3_EINVAL
        assert b"gf3_track_phase" in lib.gf3_last_error(None)
    assert lib.gf3_track_phase(eng._h, p, 1, q, None, None, None) == 0       # (both optional outputs absent)
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(out), torch.view_as_real(eng.track_phase(eq)))


def test_engine_produced_symbols():
    """The equalised symbols of a noisy fixture stream as the engine's demodulator leaves them, under a planted ramp; the same
    precondition is asserted on them."""
    from tests.test_noise_gpu import noisy_eq
    p, eng, eq = noisy_eq("g2_n4096_qpsk")
    eq = eq.cpu().numpy()
    F = eq.shape[0] // p.D
    kap = TR.kappa(p.data_carriers)
    a, e = ramps(F, p.D, (0.1, -0.05))
    rot = np.exp(1j * (a[..., None] + (e / np.abs(kap).max())[..., None] * kap)).reshape(eq.shape)
    _, phase, measured = compare("engine_eq", eng, eq * rot, p.const_points, p.data_carriers, p.D)
    assert measured.all()
    assert (np.abs(phase[..., 0] - a) + np.abs(phase[..., 1] * np.abs(kap).max() - e)).max() < 0.1


# ---- end to end through the façade ----------------------------------------------------------------------------------
TAU0 = 1.5


def restated(noisy, start, cw, p, shifts):
    """The same samples through the oracle's demodulation, the restated tracker, noise weights and the restated decoder.
    -> failed codewords (without, with the tracker)"""
    eq = orc.demod_frames(noisy, np.array([start]), p)["eq"]
    failed = []
    for e in (eq, TR.track(eq, p.const_points, p.data_carriers, p.D)[0]):
        llr = NR.soft_demap_nw(e, NR.noise_estimate(e, p.const_points, p.D), p.const_points, p.const_bits, p.D)
        bits, _, it = R.decode(shifts, llr[: cw.size].reshape(cw.shape), 50)
        failed.append(int(np.sum((bits != cw[:, : bits.shape[1]]).any(axis=1) | (it < 0))))
    return tuple(failed)


def test_facade_phase_tracking_decodes_a_packet_whose_delay_wanders():
    """Mode A2, "QCLDPC-1/2", llr_weighting "noise", 150 000 payload bits (196 codewords in one packet), white noise 12 dB
    below the signal, every data symbol of the façade's own transmit() samples delayed by tau0 sin^2(pi (l + 1/2) / D)
    samples, tau0 = 1.5: zero at both pilot blocks.

    Restated on this test's own samples, failed codewords of 196 without | with the tracker at tau0 x0.8 / x1 / x1.2:
    123 | 0,  132 | 0,  137 | 0  (the track's slope peaks at 1.610 rad at the band edge against 1.610 planted and ends at
    0.047 rad common, 0.039 rad at the band edge: what the pilot model itself leaves at 12 dB).  The test restates the counts on its own samples and asserts them before it looks at the GPU."""
    from gf3_audio_modem_amd.ldpc import shift_table
    from gf3_audio_modem_amd.OFDM import receiver
    rng = np.random.default_rng(2027)
    payload = rng.integers(0, 2, size=150_000)
    np.random.seed(23)
    tx = receiver("A2", encoding="QCLDPC-1/2")
    coded = np.asarray(tx.encode(payload))
    np.random.seed(23)
    sig = np.concatenate([np.zeros(2000), tx.transmit(payload), np.zeros(2000)])
    p = modeA2_params(np.asarray(tx.known_sequence[: tx.K * tx.mu], dtype=np.uint8))
    sh = shift_table("1/2")
    n_cw = -(-len(payload) // 768)
    cw = coded[: n_cw * 1536].astype(np.uint8).reshape(n_cw, 1536)
    start = 2000 + tx.chirp_length
    first = start + p.P * p.S
    noise = rng.normal(0, np.sqrt(np.mean(sig[2000:-2000] ** 2) / 10 ** 1.2), sig.shape)
    for scale in (0.8, 1.2, 1.0):                          # (ends on the stream the GPU receives)
        noisy = TR.delay_wander(sig, first, p.S, p.D, TAU0 * scale) + noise
        without, tracked = restated(noisy, start, cw, p, sh)
        print(f"tau0 x{scale}: restated failed codewords without the tracker {without}, with it {tracked}")
        assert without > 0 and tracked == 0

    rx = receiver("A2", encoding="QCLDPC-1/2")
    rx.llr_weighting = "noise"
    assert rx.phase_tracking is False
    out, _, _ = rx.receive(noisy)
    assert not np.array_equal(out[: len(payload)], payload)
    assert rx.last_phase_track is None and rx.last_phase_measured is None
    rx.phase_tracking = True
    out, Hs0, _ = rx.receive(noisy)
    assert out.dtype == np.int64 and Hs0.shape == (2047,)
    assert np.array_equal(out[: len(payload)], payload)
    track, measured = rx.last_phase_track, rx.last_phase_measured
    assert track.dtype == np.float64 and track.shape == (1, 180, 2) and measured.dtype == np.uint8 and measured.shape == (1, 180)
    kmax = np.abs(TR.kappa(p.data_carriers)).max()
    planted = 2 * np.pi * TAU0 * kmax / 4096
    peak = np.abs(track[0, :, 1]).max() * kmax
    print(f"slope at the band edge peaks at {peak:.3f} rad, planted {planted:.3f}; end of track {track[0, -1]}")
    assert abs(peak / planted - 1) < 0.2
    # the end pilots anchor the model, and half a symbol before them the planted wander has 0.01 % of its peak left: what
    # remains is the pilot model's own error.  The smallest cycle slip of QPSK is pi / 2 at some carrier; under a quarter
    # of that at the worst carrier is none
    assert abs(track[0, -1, 0]) + abs(track[0, -1, 1]) * kmax < np.pi / 8
    assert measured.all()
    # the static stream decodes both ways; off again, the attributes are cleared
    still = sig + noise
    for on in (True, False):
        rx.phase_tracking = on
        out, _, _ = rx.receive(still)
        assert np.array_equal(out[: len(payload)], payload)
        assert (rx.last_phase_track is not None) == on and (rx.last_phase_measured is not None) == on
    # both refusals, before any GPU work
    rx.phase_tracking, rx.fused_llr, rx.llr_weighting = True, True, "csi"
    with pytest.raises(ValueError, match="phase_tracking"):
        rx.receive(still)
    bad = receiver("A2", encoding="XOR")
    bad.phase_tracking = True
    with pytest.raises(ValueError, match="phase_tracking"):
        bad.receive(still)
