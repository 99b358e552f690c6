"""GPU parity tests: the HIP path (through the C ABI) against the golden fixtures
written from the reference and against the oracle on the same inputs.

Bars: decoded bits bit-exact; equalised symbols <= 1e-9 (north_star asks 1e-6);
channel estimates <= 1e-11 relative; slope <= 1e-11 absolute; FFT <= 1e-12 relative.
"""
import hashlib

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests.util import LOOPBACKS, engine_for, load, modeA2_params, params_of, unpack

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [1024, 2048, 4096, 8192])
def test_rfft_batch(N):
    g = load("g4_fft_mixedN")
    x = g[f"x{N}"]
    p = orc.RxParams(N=N, CP=0, P=1, D=1, lo=1, hi=N // 2 - 1, known_bits=np.zeros(N, np.uint8),
                     fit_lo=10, fit_hi=100)
    eng = engine_for(p)
    off = np.arange(x.shape[0]) * N
    X = eng.rfft_batch(x.reshape(-1), off).cpu().numpy()
    ref = g[f"X{N}"][:, : N // 2 + 1]
    assert np.abs(X - ref).max() <= 1e-12 * np.abs(ref).max()
    # unaligned (odd) offsets and the f32 storage path
    x32 = x.astype(np.float32).reshape(-1)
    eng32 = engine_for(p, in_dtype=torch.float32)
    X32 = eng32.rfft_batch(x32, [1, N + 3]).cpu().numpy()
    ref32 = np.fft.rfft(np.stack([x32[1:1 + N], x32[N + 3: 2 * N + 3]]).astype(np.float64))
    assert np.abs(X32 - ref32).max() <= 1e-12 * np.abs(ref32).max()


@pytest.mark.parametrize("name", LOOPBACKS)
def test_sync_stream_and_demod_vs_reference_fixture(name):
    g = load(name)
    p = params_of(g)
    eng = engine_for(p)
    x = torch.from_numpy(g["r"]).cuda()
    peaks, corr = eng.sync_stream(x, want_corr=True)
    assert np.array_equal(peaks.cpu().numpy(), g["peaks"])
    P = orc.matched_filter(g["r"], p)
    assert np.abs(corr.cpu().numpy() - P).max() <= 1e-11 * np.abs(P).max()
    starts = (peaks + 2)[:-1]
    o = eng.demod_frames(x, starts, want=("eq", "Hs", "He", "slope", "Hest", "status"))
    assert int(o["status"].item()) == 0
    bits = eng.unpack_bits(o["bits"]).cpu().numpy()
    assert np.array_equal(bits, unpack(g))
    assert np.array_equal(o["bits"].cpu().numpy(), orc.pack_bits(unpack(g), p.D * p.C * p.mu))
    for k in ("Hs", "He"):
        assert np.abs(o[k].cpu().numpy() - g[k]).max() <= 1e-11 * np.abs(g[k]).max()
    np.testing.assert_allclose(o["slope"].cpu().numpy(), g["slope"], rtol=0, atol=1e-11)
    scale = max(1.0, float(np.abs(g["eq"]).max()))
    assert np.abs(o["eq"].cpu().numpy() - g["eq"]).max() <= 1e-9 * scale
    np.testing.assert_allclose(o["Hest"].cpu().numpy()[0, :, ::64], g["Hest0"], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("name", ["g2_n4096_qpsk", "g8_n4096_qpsk_gr5_drift"])
@pytest.mark.parametrize("dt", [torch.float32, torch.int16, torch.uint8])
def test_narrow_sample_storage(name, dt):
    """fp32 / PCM storage: same kernels, samples widened in registers; oracle is fed
    the identically rounded samples."""
    g = load(name)
    p = params_of(g)
    r = g["r"]
    if dt == torch.float32:
        rq = r.astype(np.float32)
    elif dt == torch.int16:
        rq = np.round(r / np.abs(r).max() * 30000).astype(np.int16)
    else:
        rq = np.round(r / np.abs(r).max() * 120 + 128).astype(np.uint8)
    ref = orc.receive(rq.astype(np.float64), p)
    eng = engine_for(p, in_dtype=dt)
    x = torch.from_numpy(rq).cuda()
    peaks = eng.sync_stream(x)
    assert np.array_equal(peaks.cpu().numpy(), np.flatnonzero(ref["zeros"]))
    o = eng.demod_frames(x, (peaks + 2)[:-1], want=("eq",))
    assert np.array_equal(eng.unpack_bits(o["bits"]).cpu().numpy().reshape(-1), ref["bits"].reshape(-1))
    scale = max(1.0, float(np.abs(ref["eq"]).max()))
    assert np.abs(o["eq"].cpu().numpy() - ref["eq"]).max() <= 1e-9 * scale


def _rows_with_gaps(p, F, seed, gmax=300, mu_bits=None):
    rs = np.random.RandomState(seed)
    payload = rs.randint(0, 2, F * p.D * p.C * p.mu)
    fill = np.array([(1 + 1j) / np.sqrt(2)] * (p.K - p.C))
    frames = orc.tx_frames(payload, fill, p)
    gaps = rs.randint(0, gmax, F)
    stride = gmax + p.frame_len + 64
    rows = np.zeros((F, stride))
    for f in range(F):
        rows[f, gaps[f]: gaps[f] + p.frame_len] = frames[f]
    return rows, gaps, payload


@pytest.mark.parametrize("N,CP,mu", [(1024, 128, 2), (4096, 512, 2), (2048, 256, 6)])
def test_sync_frames_batched(N, CP, mu):
    pts, bt = orc.qpsk_table() if mu == 2 else orc.square_qam_table(mu)
    K = N // 2 - 1
    known = load("g6_realrec")["known_bits"]
    known = np.tile(known, -(-K * mu // len(known)))
    p = orc.RxParams(N=N, CP=CP, P=2, D=3, lo=1, hi=K, const_points=pts, const_bits=bt, known_bits=known,
                     fit_lo=min(500, K // 2), fit_hi=min(1000, K))
    F = 5
    rows, gaps, payload = _rows_with_gaps(p, F, seed=N)
    eng = engine_for(p, in_dtype=torch.float32, max_window=320)
    x = torch.from_numpy(rows.astype(np.float32)).cuda()
    starts, peak = eng.sync_frames(x, F, rows.shape[1], 0, 320, want_peak=True)
    assert np.array_equal(starts.cpu().numpy(), np.arange(F) * rows.shape[1] + gaps + p.Lc)
    c = orc.chirp_replica(p)
    np.testing.assert_allclose(peak.cpu().numpy(), np.full(F, np.dot(c, c)), rtol=1e-6)
    o = eng.demod_frames(x, starts, want=())
    assert np.array_equal(eng.unpack_bits(o["bits"]).cpu().numpy(), payload)   # noiseless => BER 0


@pytest.mark.parametrize("N,CP", [(1024, 128), (2048, 256), (4096, 512), (8192, 1024)])
def test_phase_slope_over_whole_band(N, CP):
    """Fit range = every carrier ([0:K]): the fit-range carriers no longer fit the FFT buffer for N = 1024 and
    8192 (they move behind the decision bytes) and fill it exactly for N = 4096.  Drifted, echoey stream;
    slope, channel estimates, equalised symbols and bits against the oracle in full mode, bits in lean mode."""
    pts, bt = orc.qpsk_table()
    K = N // 2 - 1
    known = load("g6_realrec")["known_bits"]
    known = np.tile(known, -(-K * 2 // len(known)))
    p = orc.RxParams(N=N, CP=CP, P=2, D=3, lo=1, hi=K, const_points=pts, const_bits=bt, known_bits=known,
                     fit_lo=0, fit_hi=K)
    F = 3
    rows, gaps, payload = _rows_with_gaps(p, F, seed=7 * N)
    rs = np.random.RandomState(N)
    h = np.zeros(40); h[0] = 1.0; h[3] = -0.35; h[17] = 0.2; h[39] = 0.08          # echoes inside the prefix
    x = np.concatenate([np.convolve(rows[f], h)[: rows.shape[1]] for f in range(F)])
    x = x + 0.01 * rs.randn(len(x))
    starts = np.arange(F) * rows.shape[1] + gaps + p.Lc + 1                        # one sample late: a phase ramp
    ref = orc.demod_frames(x, starts, p)
    eng = engine_for(p)
    xd = torch.from_numpy(x).cuda()
    o = eng.demod_frames(xd, starts, want=("eq", "Hs", "He", "slope"))
    np.testing.assert_allclose(o["slope"].cpu().numpy(), ref["slope"], rtol=0, atol=1e-11)
    assert np.abs(o["Hs"].cpu().numpy() - ref["Hs"]).max() <= 1e-10
    assert np.abs(o["He"].cpu().numpy() - ref["He"]).max() <= 1e-10
    assert np.abs(o["eq"].cpu().numpy().reshape(ref["eq"].shape) - ref["eq"]).max() <= 1e-6
    assert np.array_equal(eng.unpack_bits(o["bits"]).cpu().numpy().reshape(-1), ref["bits"].reshape(-1))
    lean = eng.demod_frames(xd, starts, want=())
    assert torch.equal(lean["bits"], o["bits"])


def test_sync_frames_window_rule_matches_oracle_on_multipath():
    """Window-mode peak rule == the reference rule applied to the window
    (first local extremum above 0.4*max), on an echoey channel."""
    g = load("g3_n4096_16qam_gr5")
    p = params_of(g)
    eng = engine_for(p, max_window=400)
    r = g["r"]
    x = torch.from_numpy(r).cuda()
    P = orc.matched_filter(r, p)
    for pk in g["peaks"][:-1]:
        s_true = int(pk) + 1 - (p.Lc - 1)                      # lag of the detected extremum
        lo = s_true - 150
        W = 400
        starts = eng.sync_frames(x, 1, 0, lo, lo + W)
        seg = P[lo + p.Lc - 1: lo + p.Lc - 1 + W]
        pn = seg / seg.max()
        d = np.diff(pn)
        cand = np.flatnonzero((d[:-1] * d[1:] <= 0) & (pn[1:-1] > 0.4)) + 1
        assert int(starts.item()) == lo + int(cand[0]) + p.Lc == int(pk) + 2


def test_ragged_and_empty_inputs():
    g = load("g1_n1024_qpsk")
    p = params_of(g)
    eng = engine_for(p)
    x = torch.from_numpy(g["r"]).cuda()
    o = eng.demod_frames(x, [len(g["r"]) - 100, -5], want=("status",))
    assert int(o["status"].item()) == 1 and int(o["bits"].sum()) == 0
    o = eng.demod_frames(x, [], want=())
    assert o["bits"].shape == (0, eng.bytes_per_frame)
    tail = int(g["tail"])
    assert eng.sync_stream(x[: len(x) - tail + 2]).numel() == 3
    assert eng.sync_stream(x[: len(x) - tail + 1]).numel() == 0      # the reference's except-branch quirk
    with pytest.raises(ValueError):
        eng.sync_frames(x, 1, 0, 0, 100000)


@pytest.mark.parametrize("mu", [2, 4, 6])
def test_demap_edges_and_soft(mu):
    g = load("g5_demap_edges")
    p = orc.RxParams(N=1024, CP=0, P=1, D=1, lo=1, hi=511, const_points=g[f"pts{mu}"],
                     const_bits=g[f"tbl{mu}"].astype(np.int64),
                     known_bits=np.zeros(511 * mu, np.uint8), fit_lo=10, fit_hi=100)
    eng = engine_for(p)
    sym = g[f"sym{mu}"]
    bits, idx = eng.demap_hard(sym)
    got, want = bits.cpu().numpy(), g[f"bits{mu}"]
    # the WHOLE vector, exact decision-boundary mid-points included: there the reference's abs() rounds different
    # squared distances to the same value and argmin returns the first; the engine re-measures near ties with the
    # same |.| (np_cabs in gf3rx_device.h)
    assert np.array_equal(got, want)
    noisy = sym[15:15 + 2048]
    llr = eng.soft_demap(noisy, 0.05).cpu().numpy()
    ref = orc.soft_demap_maxlog(noisy, 0.05, p)
    np.testing.assert_allclose(llr, ref.astype(np.float32), rtol=2e-6, atol=1e-6)
    assert np.array_equal((llr < 0).astype(np.uint8), want[15:15 + 2048])


@pytest.mark.parametrize("mu", [2, 4, 6])
def test_demap_near_ties_match_the_reference_distance(mu):
    """Symbols ON and within a few ulp of every decision boundary (mid-points of neighbouring constellation points,
    shifted by 0, +-1, +-2, +-5 ulp and by 1e-13 on either axis): the decision must be argmin(abs(sym - table))
    exactly as NumPy evaluates it (oracle.demap_hard), through gf3_demap_hard and through the fused kernel's
    full mode (gf3_equalise with a unit channel would rescale the symbols, so the table scan is driven directly)."""
    pts, bt = orc.qpsk_table() if mu == 2 else orc.square_qam_table(mu)
    p = orc.RxParams(N=1024, CP=0, P=1, D=1, lo=1, hi=511, const_points=pts, const_bits=bt.astype(np.int64),
                     known_bits=np.zeros(511 * mu, np.uint8), fit_lo=10, fit_hi=100)
    eng = engine_for(p)
    rs = np.random.RandomState(mu)
    i, j = np.triu_indices(len(pts), 1)
    d = np.abs(pts[i] - pts[j])
    near = d <= d.min() * 1.5                                   # horizontal, vertical and diagonal neighbours
    mid = (pts[i[near]] + pts[j[near]]) / 2
    # corners where four cells meet, and points along each boundary
    t = rs.uniform(-0.4, 0.4, size=(len(mid), 6)) * d.min()
    along = mid[:, None] + t * np.exp(1j * (np.angle(pts[i[near]] - pts[j[near]]) + np.pi / 2))[:, None]
    base = np.concatenate([mid, along.reshape(-1)])
    syms = [base]
    for k in (1, 2, 5):
        for ax in (1, 1j):
            for sgn in (1, -1):
                re = base.real if ax != 1 else np.nextafter(base.real, sgn * np.inf)
                im = base.imag if ax == 1 else np.nextafter(base.imag, sgn * np.inf)
                for _ in range(k - 1):
                    re = re if ax != 1 else np.nextafter(re, sgn * np.inf)
                    im = im if ax == 1 else np.nextafter(im, sgn * np.inf)
                syms.append(re + 1j * im)
    syms.append(base + 1e-13); syms.append(base - 1e-13j)
    sym = np.concatenate(syms)
    want, _ = orc.demap_hard(sym, p)
    got, idx = eng.demap_hard(sym)
    assert np.array_equal(got.cpu().numpy(), want)
    d2 = np.abs(sym[:, None] - pts[None, :])
    assert np.array_equal(idx.cpu().numpy(), d2.argmin(axis=1))
    # the case is not vacuous: a squared-distance argmin disagrees with the reference on some of these
    dx = sym.real[:, None] - pts.real[None, :]; dy = sym.imag[:, None] - pts.imag[None, :]
    if mu > 2:
        assert ((dx * dx + dy * dy).argmin(axis=1) != d2.argmin(axis=1)).any()


@pytest.mark.parametrize("C,mu,D", [(1, 2, 70), (4, 2, 33), (13, 2, 9), (7, 2, 12), (3, 4, 21), (1, 6, 40), (16, 2, 5)])
def test_narrow_data_bands_pack_bits_like_the_oracle(C, mu, D):
    """Data bands of a handful of carriers: an output word then spans several OFDM symbols, so the decision-byte
    ring of demod_kernel must hold ceil(32 / (C mu)) + 2 symbols.  Noisy stream; lean and full mode vs the oracle."""
    pts, bt = orc.qpsk_table() if mu == 2 else orc.square_qam_table(mu)
    N, K = 1024, 511
    known = np.tile(load("g6_realrec")["known_bits"], -(-K * mu // 4096))
    p = orc.RxParams(N=N, CP=64, P=2, D=D, lo=200, hi=200 + C, const_points=pts, const_bits=bt.astype(np.int64),
                     known_bits=known, fit_lo=100, fit_hi=400)
    F = 3
    rs = np.random.RandomState(100 * C + mu)
    payload = rs.randint(0, 2, F * D * C * mu)
    fill = rs.choice(np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) / np.sqrt(2), size=K - C)
    r = orc.tx_stream(payload, fill, p, gaps=rs.randint(0, 50, F), lead=20, tail=30)
    r = r + 0.02 * rs.randn(len(r))
    ref = orc.receive(r, p)
    eng = engine_for(p)
    x = torch.from_numpy(r).cuda()
    peaks = eng.sync_stream(x)
    assert np.array_equal(peaks.cpu().numpy(), np.flatnonzero(ref["zeros"]))
    lean = eng.demod_frames(x, (peaks + 2)[:-1])
    full = eng.demod_frames(x, (peaks + 2)[:-1], want=("eq",))
    want = orc.pack_bits(ref["bits"], D * C * mu)
    assert np.array_equal(lean["bits"].cpu().numpy(), want)
    assert np.array_equal(full["bits"].cpu().numpy(), want)
    # and the transmit kernel reads the same narrow rows
    filler = np.zeros(K, dtype=complex)
    filler[np.delete(np.arange(1, K + 1), p.data_carriers - 1) - 1] = fill
    rows = eng.tx_frames(orc.pack_bits(payload, D * C * mu), filler, out_dtype=torch.float64).cpu().numpy()
    assert np.abs(rows - orc.tx_frames(payload, fill, p)).max() <= 1e-12 * np.abs(rows).max()


def test_facade_stage_methods_match_reference_fixture():
    from gf3_audio_modem_amd.OFDM import receiver
    g = load("g8_n4096_qpsk_gr5_drift")
    p = params_of(g)
    rx = receiver(mode="A1", encoding="None", no_pilots=p.P, packet_length=p.D)
    rx.cp_length = p.CP
    rx.chirp_length = 5 * (p.N + p.CP)
    rx.lowest_bin, rx.highest_bin = p.lo, p.hi
    rx.data_carriers = np.arange(p.lo, p.hi)
    rx.data_carriers_per_symbol = p.C
    rx.data_bits_per_symbol = p.C * p.mu
    r = g["r"]
    zeros = rx.chirp_method(r)
    assert zeros.dtype == bool and len(zeros) == len(r) + rx.chirp_length - 3
    assert np.array_equal(np.flatnonzero(zeros), g["peaks"])
    sym = rx.get_symbols(r, zeros)
    assert sym.shape == (2, 2 * p.P + p.D, p.N + p.CP) and rx.no_packets == 2
    X = rx.fft(rx.remove_cp(sym))
    assert np.abs(X[0][:, 1:65] - g["X0"]).max() <= 1e-12 * np.abs(g["X0"]).max()
    data, st, en = rx.get_data(X)
    eq, Hs, He, Hest = rx.equalise(data, st, en)
    assert eq.shape == (2 * p.D, p.K) and Hest.shape == (2, p.D, p.K)
    assert np.abs(eq[:, rx.data_carriers - 1] - g["eq"]).max() <= 1e-9 * max(1, np.abs(g["eq"]).max())
    np.testing.assert_allclose(rx._last_slope, g["slope"], rtol=0, atol=1e-11)
    bits_par, hard = rx.demap(eq[:, rx.data_carriers - 1])
    assert bits_par.shape == (2 * p.D, p.C, 2) and bits_par.dtype == np.int64 and hard.shape == (2 * p.D, p.C)
    assert np.array_equal(rx.PS(bits_par), unpack(g))
    with pytest.raises(ValueError, match="Symbols must be numpy array"):
        rx.demap([1 + 1j])
    with pytest.raises(ValueError):
        rx.get_symbols(r, np.zeros_like(zeros))


def test_facade_final_system_test_known_answer(capsys):
    """The reference's own end-to-end test (Final System Test.ipynb:85-169) through the
    drop-in class: same bits, same printed BER string."""
    from gf3_audio_modem_amd.OFDM import receiver
    g = load("g6_realrec")
    r = g["wav_u8"] / 1.0                                     # notebook cell 5
    rx = receiver(mode="A2", encoding="XOR")                 # cell 6
    bits, Hstart, Hend = rx.receive(r)                       # cell 7
    out = capsys.readouterr().out
    assert "Number of received OFDM symbols:    540" in out and "Number of received bits:            1512000" in out
    assert bits.dtype == np.int64 and np.array_equal(bits, unpack(g))
    assert hashlib.sha256(bits.astype(np.uint8).tobytes()).hexdigest() == str(g["sha256_bits"])
    src = unpack(g, "src_bits", "n_src")
    ber = np.sum(bits[: len(src)] != src) / len(src)          # cell 8
    assert repr(float(ber)) == "0.023375665289067146"
    np.testing.assert_allclose(rx._last_slope, g["slope"], rtol=0, atol=1e-11)
    assert np.abs(Hstart - g["Hs0"]).max() <= 1e-11 * np.abs(g["Hs0"]).max()
    # PCM-native ingest: the raw uint8 samples give the same bits
    bits_u8, _, _ = rx.receive(g["wav_u8"])
    assert np.array_equal(bits_u8, bits)
    # ... and so does the recording taken from host memory in pieces (Engine.receive_host, two packets per piece)
    rx.host_chunk_samples = 1
    bits_c, Hs_c, He_c = rx.receive(g["wav_u8"])
    assert rx._last_ingest["chunks"] >= 2 and np.array_equal(bits_c, bits)
    assert np.abs(Hs_c - Hstart).max() <= 1e-12 * np.abs(Hstart).max() and np.abs(He_c - Hend).max() <= 1e-12 * np.abs(Hend).max()


@pytest.mark.parametrize("storage", ["int16", "float64", "float32"])
def test_peak_rule_fixture_every_sync_path(storage):
    """The reference's chirp_method outputs of g11 (amplitude ladder around 0.4 of the global maximum, a larger chirp
    suppressed by an earlier smaller one, the except-branch at tails of 0 .. 3 samples, an inverted stream) against the
    all-fp64 path, the screened path and the general screening kernel, on the PCM values and on their float copies."""
    g = load("g11_peak_rule")
    pts, bt = orc.qpsk_table()
    p = orc.RxParams(N=int(g["N"]), CP=int(g["CP"]), P=1, D=1, lo=1, hi=int(g["N"]) // 2 - 1, const_points=pts, const_bits=bt,
                     known_bits=g["known_bits"])
    eng = engine_for(p, in_dtype=getattr(torch, storage))
    for name in g["names"]:
        x = torch.from_numpy(g["r_" + str(name)].astype(storage)).cuda()
        want = g["peaks_" + str(name)]
        for mode in (1, 2, 3):
            got = eng.sync_stream(x, mode=mode).cpu().numpy()
            assert np.array_equal(got, want), (str(name), storage, mode, got, want)


def test_config1_64_frames():
    """BASELINE config 1 geometry end to end on the GPU, bit-exact vs the reference."""
    g = load("g1b_config1_64f")
    pts, bt = orc.qpsk_table()
    p = orc.RxParams(N=int(g["N"]), CP=int(g["CP"]), P=int(g["P"]), D=int(g["D"]), lo=int(g["lo"]),
                     hi=int(g["hi"]), const_points=pts, const_bits=bt, known_bits=g["known_bits"])
    F = int(g["F"])
    payload = np.random.RandomState(20261003).randint(0, 2, F * p.D * p.C * p.mu)
    r = orc.tx_stream(payload, g["fill"], p, gaps=g["gaps"], lead=int(g["lead"]), tail=int(g["tail"]))
    eng = engine_for(p)
    x = torch.from_numpy(r).cuda()
    peaks = eng.sync_stream(x)
    assert peaks.numel() == F + 1
    o = eng.demod_frames(x, (peaks + 2)[:-1])
    assert np.array_equal(eng.unpack_bits(o["bits"]).cpu().numpy(), unpack(g))


def test_config3_16qam_gr5_stream():
    """BASELINE config 3 geometry: 16-QAM, N=4096/CP=512, stream through the measured 30-tap channel
    (Handouts/gr5channel.csv, carried in the g3 fixture), stream-mode chirp sync + LS pilot equalise;
    decoded bits and BER identical to the oracle (the reference gives BER 1.1e-3 here at F=2, g3)."""
    from scipy.signal import lfilter
    g = load("g3_n4096_16qam_gr5")
    p = params_of(g, D=8)
    F = 24
    rs = np.random.RandomState(33)
    payload = rs.randint(0, 2, F * p.D * p.C * p.mu)
    fill = g["fill"]
    r = orc.tx_stream(payload, fill, p, gaps=rs.randint(0, 300, F), lead=50, tail=40)
    r = lfilter(g["channel"], 1.0, r) + 2e-4 * rs.randn(len(r))
    ref = orc.receive(r, p)
    assert len(ref["starts"]) == F
    eng = engine_for(p, in_dtype=torch.float32)
    x = torch.from_numpy(r.astype(np.float32)).cuda()
    ref32 = orc.receive(r.astype(np.float32).astype(np.float64), p)
    peaks = eng.sync_stream(x)
    assert np.array_equal(peaks.cpu().numpy(), np.flatnonzero(ref32["zeros"]))
    o = eng.demod_frames(x, (peaks + 2)[:-1])                       # MODE_SCAN: bits only, literal 16-point scan
    bits = eng.unpack_bits(o["bits"]).cpu().numpy()
    assert np.array_equal(bits, ref32["bits"])
    ber_gpu, ber_ref = np.mean(bits != payload), np.mean(ref32["bits"] != payload)
    assert ber_gpu == ber_ref and 0 < ber_gpu < 0.05
    o2 = eng.demod_frames(x, (peaks + 2)[:-1], want=("eq",))          # MODE_FULL agrees with the lean mode
    assert torch.equal(o2["bits"], o["bits"])
    assert np.abs(o2["eq"].cpu().numpy() - ref32["eq"]).max() <= 1e-9 * max(1, np.abs(ref32["eq"]).max())


def test_config3_full_size_stream():
    """BASELINE config 3 at full size (tools/config3.py: 4 096 16-QAM packets as one 321 M-sample stream through the
    measured channel).  Sync: the engine's peak list equals the ORACLE's on the same samples -- the reference's
    matched filter evaluated block-wise on the CPU (oracle.matched_filter_chunked) and its peak rule
    (global max, first extremum above 0.4, sequential suppression) on all 321 M lags.  Demod: the bits of 256
    randomly chosen packets plus the 16 WORST packets (where the reference's unwrap/slope model struggles in the
    channel's nulls) are identical to the oracle's -- parity is about matching the reference, not about BER."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("config3_tool", os.path.join(os.path.dirname(__file__), "..", "tools", "config3.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    eng, cfg, channel = tool.make_engine()
    F = 4096
    r, payload = tool.make_stream(eng, channel, F)
    res, starts, out = tool.measure(eng, cfg, r, payload, reps=1, worst=16)
    assert res["sync_offsets_as_expected_plus1"]
    pts, bt = orc.square_qam_table(4)
    known = load("g3_n4096_16qam_gr5")["known_bits"].astype(np.uint8)
    p = orc.RxParams(N=4096, CP=512, P=2, D=8, lo=1, hi=2047, const_points=pts, const_bits=bt.astype(np.int64), known_bits=known)
    rh = r.cpu().numpy().astype(np.float64)
    # ---- sync against the oracle on every lag of the stream
    Pfull = orc.matched_filter_chunked(rh, p, log2_fft=22, workers=min(16, os.cpu_count() or 1))
    want_peaks = np.flatnonzero(orc.pick_peaks(Pfull, p.Lc, len(rh), p.thresh))
    del Pfull
    got_peaks = eng.sync_stream(r).cpu().numpy()
    info = eng.sync_stream_info()
    assert info["path"] == 0 and info["cells"] < 8 * (F + 1) and info["cells_hit"] >= F + 1, info      # fp32 screen + fp64 decisions, a few cells per chirp
    assert len(want_peaks) == F + 1
    assert np.array_equal(got_peaks, want_peaks)
    assert np.array_equal(starts.cpu().numpy(), want_peaks[:-1] + 2)
    eng.sync_stream_mode(1)                                                   # and the all-fp64 path agrees
    assert np.array_equal(eng.sync_stream(r).cpu().numpy(), want_peaks)
    eng.sync_stream_mode(0)
    # ---- demod: 256 random packets + the 16 worst, each cut out with some margin and fed to the oracle
    rs = np.random.RandomState(2026)
    pick = np.unique(np.concatenate([rs.choice(F, 256, replace=False), np.asarray(res["worst_packets"]), [0, F - 1]]))
    L = cfg.M * cfg.S
    st = starts.cpu().numpy()
    segs = np.stack([rh[st[f]: st[f] + L] for f in pick])
    ref = orc.demod_frames(segs.reshape(-1), np.arange(len(pick)) * L, p)["bits"].reshape(len(pick), -1)
    got = np.unpackbits(out[torch.as_tensor(pick, device=out.device)].cpu().numpy(), axis=1)[:, : cfg.bits_per_frame]
    assert np.array_equal(ref, got)
    assert 0.0 < res["ber"] < 0.05


def test_stream_past_2_31_samples():
    """Maximum sizes: ONE stream of 2.15 G samples (27 500 config-3 packets through the measured channel), so that lag and
    sample indices pass 2^31 in every stage of the stream path.  Every chirp is found where it was put (screened and
    all-fp64 evaluation), the packets that lie wholly beyond sample 2^31 decode to the oracle's bits, and the same stream
    taken from host memory in 17 pieces gives the same peaks and the same bits."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("config3_tool", os.path.join(os.path.dirname(__file__), "..", "tools", "config3.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    eng, cfg, channel = tool.make_engine()
    F = 27500
    r, payload = tool.make_stream(eng, channel, F, seed=5)
    assert r.numel() > 2 ** 31 + 2 * cfg.frame_len
    res, starts, out = tool.measure(eng, cfg, r, payload, reps=1, warm=0, worst=4, fp64_reps=1)   # (asserts: F packets, fp64 peaks == screened)
    assert res["sync_offsets_as_expected_plus1"] and 0.0 < res["ber"] < 0.05, res
    st = starts.cpu().numpy()
    beyond = np.flatnonzero(st >= 2 ** 31)
    assert len(beyond) >= 2 and st[-1] + cfg.M * cfg.S > 2 ** 31
    pts, bt = orc.square_qam_table(4)
    known = load("g3_n4096_16qam_gr5")["known_bits"].astype(np.uint8)
    p = orc.RxParams(N=4096, CP=512, P=2, D=8, lo=1, hi=2047, const_points=pts, const_bits=bt.astype(np.int64), known_bits=known)
    pick = np.unique(np.concatenate([beyond, [beyond[0] - 1, 0], np.asarray(res["worst_packets"])]))     # (beyond[0] - 1 straddles 2^31)
    L = cfg.M * cfg.S
    segs = np.stack([r[int(st[f]): int(st[f]) + L].cpu().numpy().astype(np.float64) for f in pick])
    ref = orc.demod_frames(segs.reshape(-1), np.arange(len(pick)) * L, p)["bits"].reshape(len(pick), -1)
    got = np.unpackbits(out[torch.as_tensor(pick, device=out.device)].cpu().numpy(), axis=1)[:, : cfg.bits_per_frame]
    assert np.array_equal(ref, got)
    # ---- the stand-alone transform and the frames-mode sync at offsets past 2^31
    offs = np.array([2 ** 31 + 12345, r.numel() - cfg.N], dtype=np.int64)
    X = eng.rfft_batch(r, offs).cpu().numpy()
    for i, o in enumerate(offs):
        want = np.fft.rfft(r[int(o): int(o) + cfg.N].cpu().numpy().astype(np.float64))
        assert np.abs(X[i] - want).max() <= 1e-12 * np.abs(want).max()
    fs = eng.sync_frames(r, F, cfg.frame_len, 64 - 8, 64 + 248)      # the stream read as F rows of one packet each, a window around every chirp
    assert np.array_equal(fs.cpu().numpy(), st)
    # ---- the host-memory entry over the same samples
    host = torch.empty(r.numel(), dtype=r.dtype).pin_memory()
    host.copy_(r); torch.cuda.synchronize()
    peaks = eng.sync_stream(r)
    del r
    hr = eng.receive_host(host, chunk_samples=1 << 27)
    assert hr["info"]["chunks"] >= 16 and hr["info"]["h2d_bytes"] >= host.numel() * 4, hr["info"]
    assert torch.equal(hr["peaks"], peaks) and torch.equal(hr["bits"], out)


def test_degenerate_packets_follow_the_reference_tie_rule():
    """All-zero, NaN and Inf packets: H = 0/NaN, X/H = NaN, and the reference's argmin returns the first
    constellation point (bits 00) for every carrier.  The sign-rule fast path must fall back to the
    same answer; lean (QPSK), full and oracle agree."""
    import warnings
    g = load("g2_n4096_qpsk")
    p = params_of(g)
    n = p.M * p.S + 16
    rows = np.zeros((4, n))
    rows[1, :] = np.nan
    rows[2, :] = np.inf
    rows[3, 100:200] = 1.0                      # a packet whose pilots are partly zero: exact zeros on some carriers only
    x = rows.reshape(-1)
    starts = np.arange(4) * n
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = orc.demod_frames(x, starts, p)["bits"].reshape(4, -1)
    eng = engine_for(p)
    xd = torch.from_numpy(x).cuda()
    lean = eng.unpack_bits(eng.demod_frames(xd, starts, want=())["bits"]).cpu().numpy().reshape(4, -1)
    full = eng.unpack_bits(eng.demod_frames(xd, starts, want=("eq",))["bits"]).cpu().numpy().reshape(4, -1)
    assert not ref[:3].any() and not lean[:3].any() and not full[:3].any()
    assert np.array_equal(full, lean)
    assert np.array_equal(full[3], ref[3])


def test_lean_modes_agree_with_full_on_noisy_qpsk():
    """MODE_QPSK (sign rule, no magnitudes) == MODE_FULL (literal scan on equalised symbols) on noisy data,
    and an all-zero packet (exact ties everywhere) decodes as the reference's argmin does: label 00."""
    for name in ("g7_n4096_qpsk_drift", "g8_n4096_qpsk_gr5_drift"):
        g = load(name)
        p = params_of(g)
        eng = engine_for(p)
        x = torch.from_numpy(g["r"]).cuda()
        starts = torch.from_numpy(g["peaks"][:-1] + 2).cuda()
        lean = eng.demod_frames(x, starts)["bits"]
        full = eng.demod_frames(x, starts, want=("eq", "Hest"))["bits"]
        assert torch.equal(lean, full)
        assert np.array_equal(eng.unpack_bits(lean).cpu().numpy(), unpack(g))
    z = torch.zeros(200000, dtype=torch.float64, device="cuda")
    o = eng.demod_frames(z, [1000])
    assert int(o["bits"].sum()) == 0


@pytest.mark.parametrize("name", ["g1_n1024_qpsk", "g2_n4096_qpsk", "g3_n4096_16qam_gr5"])
def test_tx_frames_matches_reference_stream(name):
    """gf3_tx_frames against the reference's transmit() output (fixture stream r, noise-free part):
    the rows it builds, laid out with the fixture's gaps, reproduce the stream to 1e-12."""
    g = load(name)
    p = params_of(g)
    eng = engine_for(p)
    payload = unpack(g, "payload", "n_payload")
    F = len(payload) // (p.D * p.C * p.mu)
    packed = orc.pack_bits(payload, p.D * p.C * p.mu)
    filler = np.zeros(p.K, dtype=complex)
    unused = np.delete(np.arange(1, p.K + 1), p.data_carriers - 1)
    filler[unused - 1] = g["fill"]
    rows = eng.tx_frames(packed, filler, out_dtype=torch.float64).cpu().numpy()
    ref_rows = orc.tx_frames(payload, g["fill"], p)                  # bit-exact restatement of transmit()
    assert rows.shape == ref_rows.shape == (F, p.frame_len)
    assert np.abs(rows - ref_rows).max() <= 1e-12 * np.abs(ref_rows).max()
    if len(g["channel"]) == 0:                                       # and hence the reference's own stream
        r = g["r"]; pos = int(g["lead"])
        for f in range(F):
            pos += int(g["gaps"][f])
            assert np.abs(r[pos: pos + p.frame_len] - rows[f]).max() <= 1e-12 * np.abs(r).max()
            pos += p.frame_len


def test_tx_rx_round_trip_full_size():
    """Size-independent property at BASELINE config-2 size: TX -> (jitter gaps) -> sync -> demod returns
    the payload for every frame; 4096 distinct frames, 64-QAM too."""
    for mu, F in ((2, 4096), (6, 256)):
        pts, bt = orc.qpsk_table() if mu == 2 else orc.square_qam_table(mu)
        K = 2047
        known = np.tile(load("g6_realrec")["known_bits"], -(-K * mu // 4096))
        p = orc.RxParams(N=4096, CP=512, P=2, D=8, lo=1, hi=K, const_points=pts, const_bits=bt, known_bits=known)
        eng = engine_for(p, in_dtype=torch.float32, max_window=320)
        g = torch.Generator(device="cuda").manual_seed(mu)
        packed = torch.randint(0, 256, (F, eng.bytes_per_frame), dtype=torch.uint8, device="cuda", generator=g)
        gaps = torch.randint(0, 300, (F,), dtype=torch.int64, device="cuda", generator=g)
        filler = np.zeros(K, dtype=complex); filler[K - 1] = (1 - 1j) / np.sqrt(2)
        stride = 78720
        rows = eng.tx_frames(packed, filler, stride=stride, gaps=gaps, out_dtype=torch.float32)
        # the peak rule needs an interior point: start the window a few lags before the earliest chirp start
        starts = eng.sync_frames(rows, F, stride, -8, 312)
        assert torch.equal(starts, torch.arange(F, device="cuda") * stride + gaps + p.Lc)
        out = eng.demod_frames(rows, starts)["bits"]
        assert torch.equal(out, packed)


def test_facade_transmitter_reproduces_seeded_reference_stream(capsys):
    """transmitter.transmit with the same legacy-RNG seed as the fixture run gives the reference's stream."""
    from gf3_audio_modem_amd.OFDM import transmitter
    g = load("g2_n4096_qpsk")
    p = params_of(g)
    tx = transmitter(mode="A1", encoding="None", no_pilots=p.P, packet_length=p.D)
    tx.cp_length = p.CP
    tx.chirp_length = 5 * (p.N + p.CP)
    tx.lowest_bin, tx.highest_bin = p.lo, p.hi
    tx.data_carriers = np.arange(p.lo, p.hi)
    tx.data_carriers_per_symbol = p.C
    tx.unused_carriers = np.delete(tx.carriers, tx.data_carriers - 1)
    tx.data_bits_per_symbol = p.C * p.mu
    payload = unpack(g, "payload", "n_payload")
    np.random.seed(int(g["seed"]))
    sig = tx.transmit(payload)
    out = capsys.readouterr().out
    assert "Number of packets to transmit:      2" in out and "TRANSMIT" in out
    r = g["r"]
    ref = np.concatenate([r[int(g["lead"]) + int(g["gaps"][0]): int(g["lead"]) + int(g["gaps"][0]) + p.frame_len],
                          r[int(g["lead"]) + int(g["gaps"][:2].sum()) + p.frame_len:][: p.frame_len + p.Lc]])
    assert sig.shape == ref.shape
    assert np.abs(sig - ref).max() <= 1e-12 * np.abs(ref).max()


def test_facade_file_round_trip(tmp_path, monkeypatch, capsys):
    """load_file -> transmit -> receive -> save_file through the drop-in module (Final System Test flow, noiseless)."""
    from gf3_audio_modem_amd import OFDM as M
    monkeypatch.chdir(tmp_path)
    (tmp_path / "input_files").mkdir()
    blob = np.random.RandomState(4).randint(0, 256, 20000, dtype=np.uint8)
    blob.tofile(tmp_path / "input_files" / "demo.bin")
    bits = M.load_file("demo.bin")
    tx = M.transmitter(mode="A2", encoding="XOR", no_pilots=2, packet_length=8)
    np.random.seed(0)
    s = tx.transmit(bits)
    r = np.concatenate([np.zeros(100), s, np.zeros(50)])
    rx = M.receiver(mode="A2", encoding="XOR", no_pilots=2, packet_length=8)
    out_bits, Hs, He = rx.receive(r)
    assert np.array_equal(out_bits[: len(bits)], bits)
    name, data = M.save_file(out_bits)
    assert name == "demo.bin" and np.array_equal(data, blob)
    assert np.array_equal(np.fromfile(tmp_path / "output_files" / "demo_received.bin", dtype=np.uint8), blob)
    assert "File Size: 20000 bytes" in capsys.readouterr().out


def test_abi_error_paths():
    """Errors mirrored from the reference / documented in gf3rx.h: bad geometry, bad modulation,
    fit range too short, repeated data bins, wrong buffer shapes."""
    from gf3_audio_modem_amd import Engine, RxConfig, qpsk_table
    pts, bt = qpsk_table()
    known = np.zeros(8190, np.uint8)
    ok = dict(N=1024, CP=128, P=2, D=8, data_bins=np.arange(1, 511), const_points=pts, const_bits=bt,
              known_bits=known, fit_lo=100, fit_hi=400)
    Engine(RxConfig(**ok)).close()
    for bad, msg in ((dict(N=1000), "unsupported"), (dict(P=0), "P>=1"), (dict(fit_lo=509, fit_hi=510), "fit range"),
                     (dict(data_bins=np.array([5, 5, 6])), "repeated"), (dict(data_bins=np.array([0, 1])), "invalid")):
        with pytest.raises(ValueError, match=msg):
            Engine(RxConfig(**{**ok, **bad}))
    with pytest.raises(ValueError, match="Invalid Modulation"):
        Engine(RxConfig(**{**ok, "const_points": pts[:1], "const_bits": bt[:1]}))
    with pytest.raises(ValueError, match="known_bits"):
        Engine(RxConfig(**{**ok, "known_bits": np.zeros(10, np.uint8)}))
    eng = Engine(RxConfig(**ok))
    with pytest.raises(ValueError, match="bytes_per_frame"):
        eng.tx_frames(np.zeros((2, 3), np.uint8), np.zeros(511, complex))
    with pytest.raises(ValueError, match="K values"):
        eng.tx_frames(np.zeros((2, eng.bytes_per_frame), np.uint8), np.zeros(5, complex))
    with pytest.raises(ValueError, match="stride"):
        eng.tx_frames(np.zeros((2, eng.bytes_per_frame), np.uint8), np.zeros(511, complex), stride=100)
    with pytest.raises(ValueError, match="shapes"):
        eng.equalise(np.zeros((1, 8, 10), complex), np.zeros((1, 2, 511), complex), np.zeros((1, 2, 511), complex))
    # more detections than the caller's peak buffer holds: GF3_ERANGE with the true count in the message
    from gf3_audio_modem_amd.engine import Gf3Error
    g = load("g1_n1024_qpsk")
    e1 = engine_for(params_of(g))
    with pytest.raises(Gf3Error, match="exceed capacity"):
        e1.sync_stream(torch.from_numpy(g["r"]).cuda(), cap=2)
    assert e1.sync_stream(torch.from_numpy(g["r"]).cuda(), cap=3).numel() == 3        # exactly enough is fine


def test_schmidl_cox_metric():
    """gf3_schmidl_cox == the reference's schmidlcox_method on the g9 fixture (f32 and f64 storage), via the facade too."""
    from gf3_audio_modem_amd.OFDM import receiver
    g = load("g9_schmidlcox")
    r = g["r"]
    rx = receiver(mode="A1", encoding="None")
    assert rx.schmidlcox_method(r) == int(g["index"])                       # float32 samples
    assert rx.schmidlcox_method(r.astype(np.float64)) == int(g["index"])
    with pytest.raises(IndexError):
        rx.schmidlcox_method(r[:5000])


def test_real_recording_symbols_full_mode():
    """Reference default geometry (P=20, D=180, 3 packets) on the real recording: equalised symbols of the
    full-dump mode against the oracle -- 180 steps of the per-carrier phasor recurrence, 20 pilots averaged
    in the time domain -- and the bits-only mode against the full mode."""
    g = load("g6_realrec")
    p = modeA2_params(g["known_bits"])
    r = g["wav_u8"] / 1.0
    ref = orc.receive(r, p)
    eng = engine_for(p)
    x = torch.from_numpy(r).cuda()
    starts = torch.from_numpy(ref["starts"]).cuda()
    full = eng.demod_frames(x, starts, want=("eq", "Hest", "slope"))
    scale = float(np.abs(ref["eq"]).max())
    assert np.abs(full["eq"].cpu().numpy() - ref["eq"]).max() <= 1e-9 * scale
    assert np.abs(full["Hest"].cpu().numpy() - ref["Hest"]).max() <= 1e-10 * np.abs(ref["Hest"]).max()
    np.testing.assert_allclose(full["slope"].cpu().numpy(), ref["slope"], rtol=0, atol=1e-12)
    lean = eng.demod_frames(x, starts)
    assert torch.equal(lean["bits"], full["bits"])
    assert np.array_equal(eng.unpack_bits(lean["bits"]).cpu().numpy(), ref["bits"])


def test_integration_md_ctypes_stub_runs(capsys):
    """The ctypes binding printed in INTEGRATION.md (Level 2) is executed as written against the built library,
    with the facade's parameter block standing in for the reference's `self`: it must decode the real recording
    to the same bits as the maintained binding."""
    import os, re
    from gf3_audio_modem_amd.OFDM import receiver
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    md = open(os.path.join(root, "INTEGRATION.md")).read()
    block = re.search(r"## Level 2.*?```python\n(.*?)```", md, re.S).group(1)
    cwd = os.getcwd()
    os.chdir(root)                                   # the stub opens the library by its in-tree relative path
    try:
        ns = {}
        exec(block, ns)
        g = load("g6_realrec")
        rx = receiver(mode="A2", encoding="XOR")
        bits, Hs0, He0 = ns["receive"](rx, g["wav_u8"] / 1.0)
        ref_bits, ref_Hs0, ref_He0 = rx.receive(g["wav_u8"] / 1.0)
    finally:
        os.chdir(cwd)
    capsys.readouterr()
    assert np.array_equal(np.asarray(bits), np.asarray(ref_bits))
    assert np.abs(Hs0 - ref_Hs0).max() <= 1e-12 and np.abs(He0 - ref_He0).max() <= 1e-12


def test_bench_json_contract(capsys, monkeypatch):
    """bench.py --full's one JSON line (small batch, in-process): the contract keys, BER 0, exact sync, a roofline object
    whose fraction is achieved/peak, and no CPU leg when --no-cpu is given."""
    import importlib.util, json, os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gf3_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--frames", "1024", "--steps", "2", "--warmup", "1", "--no-cpu", "--no-power"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["unit"] == "samples/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert d["ber"] == 0.0 and d["sync_exact"] is True and "cpu_baseline" not in d
    assert abs(d["value"] - 1024 * 78720 * 2 / (d["ms_per_step"] * 2e-3)) <= 1e-6 * d["value"]


def test_bench_plain_run_is_lean_and_dumps_the_last_step(tmp_path, capsys, monkeypatch):
    """bench.py without --full (small batch, in-process): the headline line alone -- no secondary leg, power probe or CPU
    baseline -- over exactly --steps timed steps; --dump-outputs writes what the last timed step computed: every sync
    offset and decoded byte equal the seeded workload's own offsets and payload, and another step count writes the same."""
    import argparse, importlib.util, json, os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gf3_bench_plain", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    dumps = []
    for steps in (3, 2):
        out_dir = tmp_path / f"steps{steps}"
        monkeypatch.setattr(sys, "argv", ["bench.py", "--frames", "1024", "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out_dir)])
        bench.main()
        d = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
        assert d["steps"] == steps and d["ber"] == 0.0 and d["sync_exact"] is True
        assert abs(d["value"] - 1024 * 78720 * steps / (d["ms_per_step"] * steps * 1e-3)) <= 1e-6 * d["value"]
        for k in ("cpu_baseline", "cpu_baseline_all_cores", "cpu_baseline_config1", "screened_sync", "pcm16_storage",
                  "roofline_demod_16qam", "roofline_rfft", "roofline_demod_by_N", "roofline_stream_sync", "h2d",
                  "final_system_test", "hbm_copy_measured"):
            assert k not in d, k
        assert d["sustained_2s"] is None and d["roofline"]["power"] is None
        dumps.append({k: np.load(out_dir / f"{k}.npy") for k in ("starts", "bits_rows", "bits")})
    assert all(np.array_equal(dumps[0][k], dumps[1][k]) for k in dumps[0])
    eng, cfg, big, payload, gaps = bench.build_workload(argparse.Namespace(frames=1024, stride=78720, window=320), 0)
    exp = torch.arange(1024, device="cuda", dtype=torch.int64) * 78720 + gaps + cfg.chirp_length
    got = dumps[0]
    assert np.array_equal(got["bits_rows"], np.arange(1024))
    assert np.array_equal(got["starts"], exp.cpu().numpy().astype(np.float64))
    assert np.array_equal(got["bits"], payload.cpu().numpy().astype(np.float32))


@pytest.mark.parametrize("seed,tail", [(1, 500), (2, 1), (3, 4000)])
def test_stream_peak_picking_on_dense_candidates(seed, tail):
    """Noise-dominated streams: thousands of candidates above 0.4 max, so the candidate compaction runs over many
    blocks and the NMS over several LDS chunks with long successor chains.  The peak-picking kernels are checked in
    isolation: the reference rule (oracle.pick_peaks) applied to the engine's OWN correlation must give the same
    indices -- including the except-branch wipe when a chirp ends within the last two samples (tail = 1)."""
    import dataclasses
    g = load("g1_n1024_qpsk")
    p = dataclasses.replace(params_of(g), thresh=0.1)               # low threshold: noise extrema qualify in their thousands
    rs = np.random.RandomState(seed)
    c = orc.chirp_replica(p)
    n = 400_000
    r = 0.05 * rs.randn(n)
    for pos in (3000, 120_000, 250_000):
        r[pos: pos + p.Lc] += 0.007 * c / np.abs(c).max()           # chirps barely above the noise maximum
    r[n - tail - p.Lc: n - tail] += 0.01 * c / np.abs(c).max()      # a chirp ending `tail` samples before the end
    eng = engine_for(p, thresh=p.thresh)
    x = torch.from_numpy(r).cuda()
    peaks, corr = eng.sync_stream(x, cap=4096, want_corr=True)
    P = corr.cpu().numpy()
    zeros = orc.pick_peaks(P.copy(), p.Lc, n, p.thresh)
    want = np.flatnonzero(zeros)
    assert np.array_equal(peaks.cpu().numpy(), want)
    ncand = int(np.count_nonzero((np.diff(P / P.max())[:-1] * np.diff(P / P.max())[1:] <= 0) & ((P / P.max())[1:-1] > p.thresh)))
    assert ncand > 4096                                              # the case really is dense (several NMS chunks)
    # ... and against the ORACLE end to end (its own matched filter, its own peak rule): extrema of a noise
    # correlation are well conditioned, so both evaluations of P give the same candidates
    assert np.array_equal(peaks.cpu().numpy(), np.flatnonzero(orc.chirp_method(r, p)))


@pytest.mark.parametrize("dt,level", [(torch.float64, 1.0), (torch.uint8, 128), (torch.int16, 3)])
@pytest.mark.parametrize("n_chirps", [2.5, 7.25])
def test_constant_streams_make_every_lag_a_candidate(dt, level, n_chirps):
    """A constant stream (all ones; u8 silence at 128, which nothing recentres): the matched filter is flat over the
    full-overlap region, so rounding-noise extrema above the threshold sit on most lags -- more than half of all lags
    are candidates.  The candidate list must hold them (it is sized for every lag) and the picker must still apply
    the reference rule: peaks == oracle.pick_peaks on the engine's own correlation (the accepted positions depend on
    the last bit of P, so P itself is the only common ground with the oracle here)."""
    g = load("g1_n1024_qpsk")
    p = params_of(g)
    n = int(n_chirps * p.Lc)
    x = torch.full((n,), level, dtype=dt, device="cuda")
    eng = engine_for(p, in_dtype=dt)
    peaks, corr = eng.sync_stream(x, cap=64, want_corr=True)
    P = corr.cpu().numpy()
    want = np.flatnonzero(orc.pick_peaks(P.copy(), p.Lc, n, p.thresh))
    assert np.array_equal(peaks.cpu().numpy(), want)
    Pn = P / P.max(); d = np.diff(Pn)
    ncand = int(np.count_nonzero((d[:-1] * d[1:] <= 0) & (Pn[1:-1] > p.thresh)))
    assert ncand > 0.25 * len(P)
    ref = orc.matched_filter(np.full(n, float(level)), p)
    assert np.abs(P - ref).max() <= 1e-11 * np.abs(ref).max()


def _screen_cases():
    g1, g2 = load("g1_n1024_qpsk"), load("g2_n4096_qpsk")
    rs = np.random.RandomState(77)
    spike = np.zeros(60000); spike[31234] = 1e6; spike[5] = -3e5                       # energy in two samples
    return [("g1", params_of(g1), g1["r"], torch.float64), ("g2", params_of(g2), g2["r"], torch.float64),
            ("g2_f32", params_of(g2), g2["r"].astype(np.float32), torch.float32),
            ("noise", params_of(g1), rs.randn(150000), torch.float64),
            ("u8_dc", params_of(g1), np.clip(np.round(128 + 20 * rs.randn(90000)), 0, 255).astype(np.uint8), torch.uint8),
            ("ramp_i16", params_of(g1), (np.arange(70000) % 30000 - 15000).astype(np.int16), torch.int16),
            ("spike", params_of(g1), spike, torch.float64),
            ("ones", params_of(g1), np.ones(40000), torch.float64)]


@pytest.mark.parametrize("kernel", ["band_limited", "general"])
@pytest.mark.parametrize("case", range(8))
def test_stream_screen_error_bound_holds(case, kernel):
    """The fp32 screening pass of gf3_sync_stream (gf3rx_screen.h) against the oracle's fp64 matched filter: on every
    lag |P32 - P| must stay below the block's bound E_b -- that is what makes the screen safe.  Both kernels: the
    general one (stream mode 3; its bound is rounding only, 256 u per partition, and the arithmetic delivers a few u)
    and the band-limited one (default where the plan allows it: the bound also carries the product of the 2-norms of
    what the window and the chirp partition hold in the dropped bins -- Cauchy-Schwarz, which a stream with all its
    energy in one sample comes within 30 % of)."""
    name, p, r, dt = _screen_cases()[case]
    eng = engine_for(p, in_dtype=dt)
    eng.sync_stream_mode(3 if kernel == "general" else 2)
    x = torch.from_numpy(np.ascontiguousarray(r)).cuda()
    p32, bmax, berr, hop = eng.debug_stream_screen(x)
    P = orc.matched_filter(np.asarray(r, dtype=np.float64), p)
    p32 = p32.cpu().numpy().astype(np.float64); berr = berr.cpu().numpy().astype(np.float64); bmax = bmax.cpu().numpy()
    assert len(p32) == len(P) and hop % 2 == 0
    # (the oracle's P is itself an FFT product: allow its own rounding, ~1e-16 |r| |c|, where the bound is tiny)
    tol = 1e-13 * np.linalg.norm(np.asarray(r, dtype=np.float64)) * np.linalg.norm(orc.chirp_replica(p))
    err = np.maximum(np.abs(p32 - P) - tol, 0.0)
    per_lag = np.repeat(berr, hop)[: len(P)]
    assert (err <= per_lag).all(), (name, float((err / per_lag).max()))
    ratio = float((err / np.maximum(per_lag, 1e-300)).max())
    print(f"screen bound {name} ({kernel}): realised / bound = {ratio:.4f}, largest bound / max |P| = {berr.max() / np.abs(P).max():.2e}")
    assert ratio < (0.125 if kernel == "general" else 0.95), (name, ratio)
    nb = len(berr)
    want_max = np.array([p32[b * hop: (b + 1) * hop].max() for b in range(nb)])
    assert np.array_equal(bmax.astype(np.float64), want_max)
    if kernel == "band_limited" and name.startswith("g2"):
        # the reference geometry's chirp does qualify for the band-limited kernel: its bound shows the dropped-bin term
        eng.sync_stream_mode(3)
        berr3 = eng.debug_stream_screen(x)[2].cpu().numpy().astype(np.float64)
        assert berr.max() > 4 * berr3.max()


@pytest.mark.parametrize("kernel", ["band_limited", "general"])
def test_stream_screen_is_reproducible(kernel):
    """The screening pass twice over an 80 M-sample stream (20 000 blocks): the same lags, block maxima and bounds bit
    for bit -- a determinism check (a fixed reduction order, no atomics on values), not a race detector: what rules a race
    out is the kernel's structure (the block's bound is evaluated after the barrier, by every wave for itself from the
    completed LDS rows: gf3rx_screen.h) and the error-bound tests, which a wrong bound fails."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("config3_tool", os.path.join(os.path.dirname(__file__), "..", "tools", "config3.py"))
    c3 = importlib.util.module_from_spec(spec); spec.loader.exec_module(c3)
    eng, cfg, channel = c3.make_engine()
    r, _ = c3.make_stream(eng, channel, 1024)
    eng.sync_stream_mode(3 if kernel == "general" else 2)
    ref = None
    for _ in range(2):
        p32, bmax, berr, hop = eng.debug_stream_screen(r)
        assert bool(torch.isfinite(berr).all())
        if ref is None:
            ref = (p32.clone(), bmax.clone(), berr.clone())
        else:
            assert torch.equal(berr, ref[2]) and torch.equal(bmax, ref[1]) and torch.equal(p32, ref[0])
    peaks = [eng.sync_stream(r).cpu().numpy() for _ in range(2)]
    assert np.array_equal(peaks[0], peaks[1]) and len(peaks[0]) == 1025
    eng.close()


@pytest.mark.parametrize("name", LOOPBACKS)
def test_stream_sync_screened_equals_fp64_path(name):
    """Both evaluations of chirp_method -- fp32 screen + fp64 decisions (default) and all-fp64 overlap-save -- return
    the reference fixture's peaks, on f64, f32 and PCM storage; the screened call re-evaluates only a few cells."""
    g = load(name)
    p = params_of(g)
    r = g["r"]
    for dt, rq in ((torch.float64, r), (torch.float32, r.astype(np.float32)),
                   (torch.int16, np.round(r / np.abs(r).max() * 30000).astype(np.int16))):
        eng = engine_for(p, in_dtype=dt)
        x = torch.from_numpy(rq).cuda()
        want = np.flatnonzero(orc.chirp_method(rq.astype(np.float64), p))
        if dt == torch.float64:
            assert np.array_equal(want, g["peaks"])
        for mode in (2, 3):                                                 # (mode 0 screens from 2^23 samples on only; 3: general kernel)
            eng.sync_stream_mode(mode)
            got = eng.sync_stream(x).cpu().numpy()
            info = eng.sync_stream_info()
            assert np.array_equal(got, want)
            assert info["path"] == 0 and 0 < info["cells_hit"] <= info["cells"] <= 64 * len(want), info
        eng.sync_stream_mode(1)
        assert np.array_equal(eng.sync_stream(x).cpu().numpy(), want)
        assert eng.sync_stream_info()["path"] == 2
        eng.sync_stream_mode(0)
        assert np.array_equal(eng.sync_stream(x).cpu().numpy(), want) and eng.sync_stream_info()["path"] == 2   # short stream
        eng.sync_stream_mode(2)
        peaks, corr = eng.sync_stream(x, want_corr=True)                    # asking for P takes the fp64 path
        assert eng.sync_stream_info()["path"] == 2 and np.array_equal(peaks.cpu().numpy(), want)


def test_stream_sync_falls_back_when_the_screen_is_not_selective():
    """Noise with a low threshold: nearly every cell would have to be re-evaluated, the work list overflows and the
    call transparently takes the all-fp64 path (path 1); the peaks are the oracle's either way."""
    import dataclasses
    g = load("g1_n1024_qpsk")
    p = dataclasses.replace(params_of(g), thresh=0.1)
    rs = np.random.RandomState(5)
    n = 400_000
    r = 0.05 * rs.randn(n)
    c = orc.chirp_replica(p)
    for pos in (3000, 120_000, 250_000, n - 500 - p.Lc):
        r[pos: pos + p.Lc] += 0.008 * c / np.abs(c).max()
    eng = engine_for(p, thresh=p.thresh)
    eng.sync_stream_mode(2)
    x = torch.from_numpy(r).cuda()
    got = eng.sync_stream(x, cap=4096).cpu().numpy()
    assert eng.sync_stream_info()["path"] == 1
    assert np.array_equal(got, np.flatnonzero(orc.chirp_method(r, p)))
    # the same stream with the chirps well above the noise: selective again
    r2 = 0.0005 * rs.randn(n)
    for pos in (3000, 120_000, 250_000, n - 500 - p.Lc):
        r2[pos: pos + p.Lc] += c
    got2 = eng.sync_stream(torch.from_numpy(r2).cuda(), cap=4096).cpu().numpy()
    assert eng.sync_stream_info()["path"] == 0
    assert np.array_equal(got2, np.flatnonzero(orc.chirp_method(r2, p)))


@pytest.mark.parametrize("mu,dt", [(2, torch.float64), (4, torch.float32), (6, torch.float64)])
def test_known_channel_zero_forcing(mu, dt):
    """gf3_equalise_known_h (the reference's older known-H flow, Weekend Challenge.ipynb cells 9-17) against the
    oracle's restatement of the formula: FFT(rx)/fft(h, N), data carriers, demap -- stream through the measured
    30-tap channel with sample-exact symbol offsets; noiseless, so the payload comes back too.  Parity unpinned
    (no reference function survives); the comparison is engine vs oracle on the same samples."""
    from scipy.signal import lfilter
    g = load("g3_n4096_16qam_gr5")
    pts, bt = orc.qpsk_table() if mu == 2 else orc.square_qam_table(mu)
    K = 2047
    known = np.tile(g["known_bits"].astype(np.uint8), -(-K * mu // len(g["known_bits"])))
    p = orc.RxParams(N=4096, CP=512, P=1, D=5, lo=100, hi=1500, const_points=pts, const_bits=bt.astype(np.int64), known_bits=known)
    rs = np.random.RandomState(mu)
    F = 2
    payload = rs.randint(0, 2, F * p.D * p.C * p.mu)
    fill = rs.choice(orc.qpsk_table()[0], size=K - p.C)
    r = lfilter(g["channel"], 1.0, orc.tx_stream(payload, fill, p, lead=37, tail=50))
    if dt == torch.float32:
        r = r.astype(np.float32)
    # data symbols of packet f start (past their prefix) at lead + f frame_len + Lc + (P + l) S + CP
    offs = np.array([37 + f * p.frame_len + p.Lc + (p.P + l) * p.S + p.CP for f in range(F) for l in range(p.D)])
    h = 2.0 * g["channel"]                                  # the transmitter's x2 symbol gain (OFDM.py:256) is part of "the channel"
    ref_eq, ref_bits = orc.zf_known_h(np.asarray(r, dtype=np.float64), offs, h, p)
    eng = engine_for(p, in_dtype=dt)
    eq, bits, idx = eng.equalise_known_h(torch.from_numpy(r).cuda(), offs, h)
    assert np.abs(eq.cpu().numpy() - ref_eq).max() <= 1e-9 * max(1.0, np.abs(ref_eq).max())
    assert np.array_equal(bits.cpu().numpy(), ref_bits)
    if dt == torch.float64:
        assert np.array_equal(bits.cpu().numpy().reshape(-1), payload)       # noiseless + known channel => BER 0


@pytest.mark.parametrize("mu", [4, 6])
def test_soft_demap_generic_grid_kernel(mu):
    """Square Gray QAM whose label bits are listed in reverse order (the Q axis owns the leading bits): still a
    separable grid, but not the binary-indexed layout the straight-line kernel is specialised for -- the scalar-steered
    generic grid kernel runs.  LLRs against the oracle's max-log formula, signs against the hard decisions."""
    pts, bt = orc.square_qam_table(mu)
    bt = bt[:, ::-1].copy()
    p = orc.RxParams(N=1024, CP=0, P=1, D=1, lo=1, hi=511, const_points=pts, const_bits=bt.astype(np.int64),
                     known_bits=np.zeros(511 * mu, np.uint8), fit_lo=10, fit_hi=100)
    eng = engine_for(p)
    rs = np.random.RandomState(mu)
    sym = pts[rs.randint(0, len(pts), 5000)] + 0.1 * (rs.randn(5000) + 1j * rs.randn(5000))
    llr = eng.soft_demap(sym, 0.02).cpu().numpy()
    ref = orc.soft_demap_maxlog(sym, 0.02, p)
    np.testing.assert_allclose(llr, ref.astype(np.float32), rtol=2e-6, atol=1e-6)
    hard, _ = eng.demap_hard(sym)
    assert np.array_equal((llr < 0).astype(np.uint8), hard.cpu().numpy())
    assert np.array_equal(hard.cpu().numpy(), orc.demap_hard(sym, p)[0])


@pytest.mark.parametrize("mode", [1, 2])
def test_stream_sync_degenerate_streams(mode):
    """Streams shorter than a chirp, all-zero streams (P = 0 everywhere: the reference divides 0 by 0 and finds nothing)
    and a lone partial chirp, through the all-fp64 path (mode 1) and the screened path (mode 2): the oracle's peaks."""
    import warnings
    g = load("g1_n1024_qpsk")
    p = params_of(g)
    c = orc.chirp_replica(p)
    rs = np.random.RandomState(9)
    cases = [np.zeros(50), np.zeros(3 * p.Lc), rs.randn(37), rs.randn(p.Lc // 3),
             np.concatenate([np.zeros(10), c[: p.Lc // 2], np.zeros(500)]),
             np.concatenate([np.zeros(700), c, np.zeros(2)]), np.concatenate([np.zeros(700), c, np.zeros(1)])]
    eng = engine_for(p)
    eng.sync_stream_mode(mode)
    for r in cases:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = np.flatnonzero(orc.chirp_method(r, p))
        got = eng.sync_stream(torch.from_numpy(r).cuda()).cpu().numpy()
        assert np.array_equal(got, want), (mode, len(r), got, want)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_stream_sync_non_finite_huge_and_tiny_samples(mode):
    """`P /= max(P)` with `np.amax` (OFDM.py:359): one NaN or Inf sample makes the maximum NaN and the reference finds
    nothing anywhere in the stream -- so do the all-fp64 path (a NaN-propagating maximum) and the screened paths (a
    window whose fp32 energy is not finite sends the call to the fp64 path).  The same exit serves finite samples
    beyond fp32's range, and samples so small that fp32 sees silence fall back through the empty bound: the peaks of
    the stream scaled by 1e30 / 1e-45 are the peaks of the stream (1e-30 is still within fp32's reach: screened).  Inverted and negative-only streams for good measure."""
    import warnings
    g = load("g1_n1024_qpsk")
    p = params_of(g)
    c = orc.chirp_replica(p)
    rs = np.random.RandomState(4)
    n = 60000
    base = 0.01 * rs.randn(n); base[5000:5000 + p.Lc] += c; base[30000:30000 + p.Lc] += c
    cases = {"nan": base.copy(), "inf": base.copy(), "ninf": base.copy(), "huge": base * 1e30, "small": base * 1e-30, "tiny": base * 1e-45,
             "inverted": -base, "negative_only": -np.abs(base), "neg_dc": base - 5.0, "neg_const": np.full(40000, -3.0)}
    cases["nan"][12345] = np.nan; cases["inf"][23456] = np.inf; cases["ninf"][23456] = -np.inf
    eng = engine_for(p)
    eng.sync_stream_mode(mode)
    for name, r in cases.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = np.flatnonzero(orc.chirp_method(r, p))
        got = eng.sync_stream(torch.from_numpy(r).cuda(), cap=len(r) + p.Lc).cpu().numpy()
        assert np.array_equal(got, want), (name, mode, eng.sync_stream_info(), got[:8], want[:8])
        if name in ("nan", "inf", "ninf"):
            assert len(want) == 0
        if name in ("huge", "small", "tiny"):
            assert len(want) == 2
        if mode >= 2 and name in ("nan", "inf", "ninf", "huge", "tiny"):
            assert eng.sync_stream_info()["path"] == 1, (name, eng.sync_stream_info())


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_stream_sync_with_interferers(mode):
    """Chirps under a loud tone outside the chirp's band (20 kHz: everything the band-limited screen drops), under one
    inside it (1 kHz), under both, and under white noise as loud as the chirp: the bounds grow with what the windows hold
    outside the band, more cells are re-evaluated or the call falls back -- the peaks are the oracle's on every path."""
    g = load("g1_n1024_qpsk")
    p = params_of(g)
    c = orc.chirp_replica(p)
    rs = np.random.RandomState(12)
    n = 90000
    t = np.arange(n)
    base = np.zeros(n)
    for pos in (4000, 31000, 64000):
        base[pos: pos + p.Lc] += c
    cases = {"tone_out": base + 5.0 * np.sin(2 * np.pi * 20000 / 48000 * t), "tone_in": base + 1.0 * np.sin(2 * np.pi * 1000 / 48000 * t + 0.3),
             "both": base + 3.0 * np.sin(2 * np.pi * 20000 / 48000 * t) + 0.5 * np.sin(2 * np.pi * 3000 / 48000 * t),
             "noise": base + 0.15 * rs.randn(n), "impulses": base + 40.0 * (rs.rand(n) < 2e-4)}
    eng = engine_for(p)
    eng.sync_stream_mode(mode)
    for name, r in cases.items():
        want = np.flatnonzero(orc.chirp_method(r, p))
        got = eng.sync_stream(torch.from_numpy(r).cuda(), cap=len(r) + p.Lc).cpu().numpy()
        assert np.array_equal(got, want), (name, mode, eng.sync_stream_info(), got[:8], want[:8])
        assert len(want) >= 1, name


def test_new_abi_error_paths():
    """gf3_sync_stream_mode / gf3_equalise_known_h reject what the header says they reject."""
    g = load("g1_n1024_qpsk")
    eng = engine_for(params_of(g))
    for bad in (-1, 4):
        with pytest.raises(ValueError, match="mode"):
            eng.sync_stream_mode(bad)
    x = torch.zeros(5000, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="n_taps"):
        eng.equalise_known_h(x, [0], np.zeros(0))
    with pytest.raises(ValueError, match="n_taps"):
        eng.equalise_known_h(x, [0], np.ones(5000))
    eq, bits, idx = eng.equalise_known_h(x, [], np.ones(3))                    # no symbols: nothing to do
    assert eq.shape[0] == 0


def test_two_threads_two_streams_share_one_context():
    """include/gf3rx.h: no call writes into a context, so concurrent calls on one context are safe.  Two host threads,
    each on its own HIP stream, run stream sync (different per-call modes) + demod on different inputs through ONE
    engine; each must get exactly what the same calls give alone, its own diagnostics, and its own error text.
    (Run once: it checks results; it is not a stress loop.)"""
    import threading
    g = load("g2_n4096_qpsk")
    p = params_of(g)
    eng = engine_for(p)
    xa = torch.from_numpy(g["r"]).cuda()
    xb = torch.cat([torch.zeros(777, dtype=torch.float64, device="cuda"), 0.5 * xa])   # another stream: shifted, scaled

    def work(x, mode):
        peaks, info = eng.sync_stream(x, mode=mode, want_info=True)
        bits = eng.demod_frames(x, (peaks + 2)[:-1])["bits"]
        return peaks.cpu().numpy(), bits.cpu().numpy(), info

    alone = [work(xa, 1), work(xb, 2)]
    assert np.array_equal(alone[0][0], g["peaks"]) and np.array_equal(alone[1][0], g["peaks"] + 777)
    assert alone[0][2]["path"] == 2 and alone[1][2]["path"] in (0, 1)
    got, errs, texts = [None, None], [None, None], [None, None]
    go = threading.Barrier(2)

    def run(i, x, mode):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                go.wait()
                for _ in range(3):
                    got[i] = work(x, mode)
                    assert eng.sync_stream_info() == got[i][2]                 # this thread's own last call
                if i == 0:                                                     # a failing call in ONE thread ...
                    with pytest.raises(Exception) as ei:
                        eng.sync_stream(x, cap=1, mode=mode)
                    texts[0] = str(ei.value)
                else:
                    texts[1] = eng.lib.gf3_last_error(eng._h).decode()         # ... leaves the other's error text alone
                torch.cuda.current_stream().synchronize()
        except BaseException as e:                                             # noqa: BLE001 (reported below)
            errs[i] = e

    th = [threading.Thread(target=run, args=(0, xa, 1)), threading.Thread(target=run, args=(1, xb, 2))]
    for t in th: t.start()
    for t in th: t.join()
    assert errs == [None, None], errs
    for i in range(2):
        assert np.array_equal(got[i][0], alone[i][0]) and np.array_equal(got[i][1], alone[i][1]) and got[i][2] == alone[i][2]
    assert "exceed capacity" in texts[0] and "exceed capacity" not in texts[1]


# ---------------------------------------------------------------------------------------------------------------
# host ingest: Engine.receive_host (gf3_sync_chunk + gf3_sync_decide) -- the stream cut into pieces, the reference's
# global rule intact
# ---------------------------------------------------------------------------------------------------------------
def _config1_case():
    g = load("g1b_config1_64f")
    pts, bt = orc.qpsk_table()
    p = orc.RxParams(N=int(g["N"]), CP=int(g["CP"]), P=int(g["P"]), D=int(g["D"]), lo=int(g["lo"]),
                     hi=int(g["hi"]), const_points=pts, const_bits=bt, known_bits=g["known_bits"])
    F = int(g["F"])
    payload = np.random.RandomState(20261003).randint(0, 2, F * p.D * p.C * p.mu)
    r = orc.tx_stream(payload, g["fill"], p, gaps=g["gaps"], lead=int(g["lead"]), tail=int(g["tail"]))
    return g, p, F, r


@pytest.mark.parametrize("storage", ["f64_pageable", "f32_pinned"])
def test_receive_host_chunked_equals_one_shot_and_reference(storage):
    """BASELINE config 1 (64 frames, the reference's own bits in the g1b fixture) from HOST memory in 33 pieces of
    two packets each -- pageable (staged through pinned buffers two pieces ahead) and pinned -- : peaks and bits of the
    one-shot device path and of the reference."""
    g, p, F, r = _config1_case()
    dt = torch.float64 if storage.startswith("f64") else torch.float32
    eng = engine_for(p, in_dtype=dt)
    if storage == "f32_pinned":
        host = torch.from_numpy(r.astype(np.float32)).pin_memory()
        ref_bits = orc.receive(r.astype(np.float32).astype(np.float64), p)["bits"]
    else:
        host, ref_bits = r, unpack(g)
    out = eng.receive_host(host, chunk_samples=1)                       # (raised to two packets per piece)
    info = out["info"]
    assert info["chunks"] >= 4 and info["pinned_input"] == (storage == "f32_pinned") and info["source"] == ("pinned" if storage == "f32_pinned" else "pageable, staged"), info
    x = torch.as_tensor(host).cuda()
    one = eng.sync_stream(x)
    assert torch.equal(out["peaks"], one) and out["peaks"].numel() == F + 1
    bits_one = eng.demod_frames(x, (one + 2)[:-1])["bits"]
    assert torch.equal(out["bits"], bits_one)
    assert np.array_equal(eng.unpack_bits(out["bits"]).cpu().numpy(), ref_bits)
    assert info["second_look_chunks"] == 0 and info["second_look_packets"] == 0, info     # a clean stream needs no second look
    assert info["h2d_bytes"] == len(r) * x.element_size()                                 # every sample crossed PCIe once
    # ... and as ONE piece it is the one-shot path
    out1 = eng.receive_host(host, chunk_samples=1 << 24)
    assert out1["info"]["chunks"] == 1 and torch.equal(out1["peaks"], one) and torch.equal(out1["bits"], bits_one)


def _crafted_stream(p, lead_zeros, lead_noise=0.0):
    """[lead | weak bare chirp W1 (0.3) overlapping the chirp of packet 0 sent at HALF amplitude | 21 000 zeros |
    packets 1..5 at full amplitude | terminating chirp | tail].  While only the first piece has been seen the maximum
    is packet 0's (0.5): W1 (0.3 / 0.5 = 0.6 > 0.4) is a candidate, comes first and suppresses packet 0's chirp, which
    lies within Lc of it.  A later piece raises the maximum to 1.0: W1 (0.3) dies and packet 0's chirp (0.5) stands."""
    rs = np.random.RandomState(77)
    F = 6
    payload = rs.randint(0, 2, F * p.D * p.C * p.mu)
    fill = (np.array([1 + 1j]) / np.sqrt(2))[: p.K - p.C] if p.K > p.C else np.zeros(0, complex)
    rows = orc.tx_frames(payload, fill, p)                               # [F, Lc + M S]
    chirp = orc.chirp_replica(p)
    Lc = p.Lc
    s = np.concatenate([np.zeros(lead_zeros + Lc // 2), 0.5 * rows[0], np.zeros(21000), rows[1:].reshape(-1), chirp, np.zeros(40)])
    s[lead_zeros: lead_zeros + Lc] += 0.3 * chirp / 0.2 * 0.2            # W1 starts Lc/2 before packet 0's chirp
    s[lead_zeros:] += 1e-5 * rs.randn(len(s) - lead_zeros)              # (the lead-in stays EXACTLY zero: no positive maximum there)
    if lead_noise:
        s[:lead_zeros] = lead_noise * rs.randn(lead_zeros)               # ... or holds noise only: a noise-sized maximum
    return s, payload


@pytest.mark.parametrize("lead_zeros,list_cap,lead_noise", [(50, None, 0.0), (50, 4, 0.0), (45000, None, 0.0), (45000, 64, 1e-3)])
def test_receive_host_later_piece_changes_earlier_decisions(lead_zeros, list_cap, lead_noise):
    """The hard case of the global-max rule (OFDM.py:359): a later piece raises the maximum, which kills a candidate
    the first piece had accepted AND thereby un-suppresses another one -- a detection the provisional pass never
    demodulated (second look at that packet).  With 45 000 leading zeros the first piece has no positive maximum at
    all, so every one of its lags qualifies and the list overflows; with leading noise (and a small list) it overflows
    on a noise-sized maximum: either way only the piece's own maximum is kept, and as it cannot reach 0.4 x the final
    maximum the piece is never looked at again.  A list capacity of 4 on the ordinary stream overflows on pieces that DO
    hold chirps: those are copied and listed again at the end.  Expected: exactly the oracle's detections and bits."""
    g = load("g1_n1024_qpsk")
    p = params_of(g)
    r, payload = _crafted_stream(p, lead_zeros, lead_noise)
    ref = orc.receive(r, p)
    want_peaks = np.flatnonzero(ref["zeros"])
    assert len(want_peaks) == 7                                         # packets 0..5 + the terminating chirp: W1 is NOT among them
    eng = engine_for(p)
    out = eng.receive_host(r, chunk_samples=1, list_cap=list_cap)
    info = out["info"]
    assert info["chunks"] >= 4, info
    assert np.array_equal(out["peaks"].cpu().numpy(), want_peaks), (out["peaks"], want_peaks, info)
    assert np.array_equal(eng.unpack_bits(out["bits"]).cpu().numpy(), ref["bits"])
    assert np.array_equal(ref["bits"], payload)
    x = torch.from_numpy(r).cuda()
    assert torch.equal(eng.sync_stream(x), out["peaks"])                # the one-shot device path agrees
    if lead_zeros == 50 and list_cap is None:
        # the provisional pass accepted W1, demodulated what followed it, and had to drop that at the end;
        # packet 0 was only found with the final maximum
        assert info["provisional_detections_dropped"] >= 1 and info["second_look_packets"] >= 1, info
    elif lead_zeros == 50:
        assert info["second_look_chunks"] >= 1, info                    # overflowing pieces that hold chirps: listed again
    else:
        assert info.get("overflow_pieces_below_threshold", 0) >= 1 and info["second_look_chunks"] == 0, info   # a silent / noisy lead-in costs nothing


def test_receive_host_fails_where_the_reference_fails():
    g = load("g1_n1024_qpsk")
    p = params_of(g)
    eng = engine_for(p)
    rs = np.random.RandomState(5)
    with pytest.raises(ValueError):                                     # no chirp at all: np.vstack([]) in the reference
        eng.receive_host(1e-3 * rs.randn(150000), chunk_samples=1)
    r = g["r"]
    cut = r[: int(g["peaks"][0]) + 2 + 3 * p.S]                         # first packet cut short, then a chirp glued on
    bad = np.concatenate([cut, orc.chirp_replica(p), np.zeros(10)])
    with pytest.raises(ValueError):
        orc.receive(bad, p)
    with pytest.raises(ValueError):
        eng.receive_host(bad, chunk_samples=1)


# ---------------------------------------------------------------------------------------------------------------
# the two-phase demodulation of long packets, few at a time (gf3_demod_frames_ex; gf3rx_demod_split.hip)
# ---------------------------------------------------------------------------------------------------------------
def _same_as_one_launch(eng, x, starts, want, rows=None):
    """rows: the packets whose dumps are compared (a ragged packet's are left unwritten by both paths)"""
    one = eng.demod_frames(x, starts, want=want, split=False)
    two = eng.demod_frames(x, starts, want=want, split=True)
    assert torch.equal(one["bits"], two["bits"])
    rows = slice(None) if rows is None else rows
    for k in ("Hs", "He", "slope"):                                 # the same doubles: the estimate stage IS the one-launch kernel's
        if k in want:
            assert torch.equal(one[k][rows], two[k][rows]), k
    for k in ("eq", "Hest"):                                        # phasor at a chunk's first symbol: direct instead of by recurrence
        if k in want:
            a, b = one[k].cpu().numpy(), two[k].cpu().numpy()
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, float(np.abs(a).max())), k
    if "status" in want:
        assert int(one["status"].item()) == int(two["status"].item())
    return one, two


@pytest.mark.parametrize("storage", ["u8", "f64"])
def test_split_path_on_the_real_recording(storage):
    """The reference's own test geometry (P = 20, D = 180, three packets): the library picks the two-phase form by
    itself, and it returns the one-launch path's Hs / He / slope bit for bit, its bits, eq within 1e-12 -- and the
    reference's bits."""
    g = load("g6_realrec")
    p = modeA2_params(g["known_bits"])
    r = g["wav_u8"] if storage == "u8" else g["wav_u8"] / 1.0
    eng = engine_for(p, in_dtype=torch.uint8 if storage == "u8" else torch.float64)
    plan = eng.demod_plan(3)
    assert plan["split"] and plan["chunks"] >= 4 and (plan["Dc"] * p.C * p.mu) % 32 == 0, plan
    # the rule of gf3rx.h (mode 0): two-phase while a packet cuts into two chunks or more and F <= 2 x CUs
    assert eng.demod_plan(2 * eng.n_cu)["split"] == (eng.demod_plan(2 * eng.n_cu)["chunks"] >= 2)
    assert not eng.demod_plan(2 * eng.n_cu + 1)["split"] and not eng.demod_plan(65536)["split"]
    x = torch.from_numpy(r).cuda()
    starts = torch.from_numpy(np.asarray(g["peaks"][:-1]) + 2).cuda()
    one, two = _same_as_one_launch(eng, x, starts, ("eq", "Hest", "Hs", "He", "slope"))
    lean_one, lean_two = _same_as_one_launch(eng, x, starts, ("Hs", "He", "slope"))
    assert torch.equal(lean_two["bits"], two["bits"])
    auto = eng.demod_frames(x, starts)                               # no dumps asked for: state lives in the workspace
    assert torch.equal(auto["bits"], two["bits"])
    bits = eng.unpack_bits(auto["bits"]).cpu().numpy()
    ref = orc.receive(g["wav_u8"] / 1.0, p)
    assert np.array_equal(bits, ref["bits"])
    assert np.abs(two["eq"].cpu().numpy() - ref["eq"]).max() <= 1e-9 * float(np.abs(ref["eq"]).max())


@pytest.mark.parametrize("name", LOOPBACKS)
def test_split_path_on_the_loopback_fixtures(name):
    """Every reference fixture through the forced two-phase form (short packets: one chunk per packet, the estimate
    stage and the state hand-over are what is exercised), all three modes of the data stage."""
    g = load(name)
    p = params_of(g)
    eng = engine_for(p)
    x = torch.from_numpy(g["r"]).cuda()
    starts = torch.from_numpy(np.asarray(g["peaks"][:-1]) + 2).cuda()
    one, two = _same_as_one_launch(eng, x, starts, ("eq", "Hs", "He", "slope", "Hest", "status"))
    lean = eng.demod_frames(x, starts, split=True)
    assert torch.equal(lean["bits"], two["bits"])
    assert np.array_equal(eng.unpack_bits(lean["bits"]).cpu().numpy(), unpack(g))
    assert np.abs(two["eq"].cpu().numpy() - g["eq"]).max() <= 1e-9 * max(1.0, float(np.abs(g["eq"]).max()))


@pytest.mark.parametrize("N,C,mu,D,P,dt", [(1024, 333, 2, 40, 3, torch.float64),      # q = 16: chunks of 16, 16, 8; odd word count
                                           (1024, 7, 4, 50, 1, torch.float32),        # 28 bits per symbol: q = 8, words span symbols
                                           (2048, 1, 2, 70, 2, torch.int16),          # one carrier: q = 16
                                           (4096, 1400, 2, 37, 5, torch.float32),     # the reference band, D odd
                                           (8192, 4095, 6, 12, 2, torch.float32),     # 64-QAM, every carrier, N = 8192
                                           (2048, 500, 4, 9, 4, torch.uint8)])        # 16-QAM on 8-bit samples
def test_split_path_round_trip_geometries(N, C, mu, D, P, dt):
    """TX -> two-phase RX returns the payload, and equals the one-launch path, for chunk lengths forced by
    32 / gcd(C mu, 32), partial last words, words spanning several symbols, every FFT size and sample storage."""
    pts, bt = orc.qpsk_table() if mu == 2 else orc.square_qam_table(mu)
    K = N // 2 - 1
    known = np.tile(load("g6_realrec")["known_bits"], -(-K * mu // 4096))
    lo = 1 if C == K else 50
    p = orc.RxParams(N=N, CP=N // 16, P=P, D=D, lo=lo, hi=lo + C, const_points=pts, const_bits=bt.astype(np.int64),
                     known_bits=known, fit_lo=60, fit_hi=min(400, K))
    F = 3
    eng_tx = engine_for(p, in_dtype=torch.float64)
    gen = torch.Generator(device="cuda").manual_seed(N + C + mu)
    packed = torch.randint(0, 256, (F, eng_tx.bytes_per_frame), dtype=torch.uint8, device="cuda", generator=gen)
    nbits = D * C * mu
    if nbits % 8:
        packed[:, -1] &= (0xFF << (8 - nbits % 8)) & 0xFF             # bits past the payload stay zero
    filler = np.zeros(K, dtype=complex)
    rs = np.random.RandomState(C)                                    # (random filler: a constant one is an impulse in time, which 8-bit storage would clip everything else under)
    filler[np.delete(np.arange(K), p.data_carriers - 1)] = rs.choice(np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) / np.sqrt(2), size=K - C)
    rows = eng_tx.tx_frames(packed, filler, out_dtype=torch.float64)
    if dt in (torch.int16, torch.uint8):
        amp = float(rows.abs().max())
        q = rows * ((20000.0 if dt == torch.int16 else 100.0) / amp)
        rows_q = (q.round() + (128 if dt == torch.uint8 else 0)).to(dt)
    else:
        rows_q = rows.to(dt)
    eng = engine_for(p, in_dtype=dt)
    starts = torch.arange(F, device="cuda") * rows.shape[1] + p.Lc
    plan = eng.demod_plan(F, split=True)
    assert (plan["Dc"] * C * mu) % 32 == 0 or plan["chunks"] == 1, plan
    one, two = _same_as_one_launch(eng, rows_q, starts, ("eq", "Hs", "He", "slope", "status"))
    lean = eng.demod_frames(rows_q, starts, split=True)
    assert torch.equal(lean["bits"], packed)
    assert torch.equal(two["bits"], packed)


def test_split_path_ragged_packet_and_status():
    """A packet that runs past the stream decodes to zero bits and raises the status bit in the two-phase form too
    (the estimate stage zeroes the row, the data stage leaves it alone)."""
    g = load("g7_n4096_qpsk_drift")
    p = params_of(g)
    eng = engine_for(p)
    x = torch.from_numpy(g["r"]).cuda()
    good = np.asarray(g["peaks"][:-1]) + 2
    starts = torch.from_numpy(np.concatenate([good, [len(g["r"]) - 100, -5]])).cuda()
    one, two = _same_as_one_launch(eng, x, starts, ("slope", "Hs", "He", "status"), rows=slice(0, len(good)))
    assert int(two["status"].item()) == 1
    assert int(two["bits"][len(good):].sum()) == 0
    assert np.array_equal(eng.unpack_bits(two["bits"][: len(good)]).cpu().numpy(), unpack(g))


def test_notebook_calls_graph_output_channel_response_save_file(tmp_path, monkeypatch, capsys):
    """Cells 7-9 of `Final System Test.ipynb` as the notebook makes them, on the GPU path: receive(r, graph_output=True)
    (OFDM.py:615-654: the full-dump mode of the demodulator feeds the two plots), save_file(rx_bits) (:766-794) and
    channel_response(Hstart) (:553-577).  What the unmodified reference prints, returns and writes for these calls is in
    the g6 fixture (tests/golden/make_golden.py ran them)."""
    import os
    import matplotlib
    matplotlib.use("Agg", force=True)
    import matplotlib.pyplot as plt
    plt.switch_backend("Agg")
    from gf3_audio_modem_amd.OFDM import receiver, save_file
    g = load("g6_realrec")
    monkeypatch.chdir(tmp_path)
    r = g["wav_u8"] / 1.0                                            # notebook cell 5
    rx = receiver(mode="A2", encoding="XOR")
    capsys.readouterr()
    rx_bits, Hstart, Hend = rx.receive(r, graph_output=True)         # cell 7
    assert capsys.readouterr().out == str(g["receive_stdout"])
    assert hashlib.sha256(rx_bits.astype(np.uint8).tobytes()).hexdigest() == str(g["sha256_bits"])
    assert rx_bits.dtype == np.int64 and len(rx_bits) == int(g["n_bits"])
    assert np.abs(Hstart - g["Hs0"]).max() <= 1e-11 * np.abs(g["Hs0"]).max()
    assert np.abs(Hend - g["He0"]).max() <= 1e-11 * np.abs(g["He0"]).max()
    for f in g["plots_receive"].tolist():
        assert os.path.getsize(f) > 1000, f
    src = np.unpackbits(g["src_bits"])[: int(g["n_src"])]            # cell 8
    errs = np.sum(abs(src.astype(np.int64) - rx_bits[: len(src)]))
    assert "{}".format(errs / len(src)) == str(g["ber_str"])
    name, data = save_file(rx_bits)
    assert capsys.readouterr().out == str(g["save_stdout"])
    assert name == str(g["save_name"]) and len(data) == int(g["save_data_len"])
    assert hashlib.sha256(np.asarray(data, dtype=np.uint8).tobytes()).hexdigest() == str(g["save_data_sha256"])
    for f in g["save_files"].tolist():
        assert hashlib.sha256(open(f, "rb").read()).hexdigest() == str(g["save_data_sha256"]), f
    rx.channel_response(Hstart)                                      # cell 9
    for f in g["plots_channel"].tolist():
        assert os.path.getsize(f) > 1000, f
    plt.close("all")


@pytest.mark.parametrize("C,mu,D", [(1400, 2, 180), (7, 3, 5), (333, 2, 3)])
def test_unpack_decode_kernel_matches_numpy(C, mu, D):
    """gf3_unpack_bits (PS + decode, OFDM.py:504-505, 541-544): int64 0/1 in the reference's order, XOR with
    tile(mask)[:len]; into device memory and straight into pinned host memory; odd bits-per-packet (padded rows);
    pageable host memory is refused."""
    import ctypes
    pts, bt = orc.qpsk_table() if mu == 2 else (np.exp(2j * np.pi * np.arange(8) / 8), np.array([[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)]))
    K = 2047
    known = np.tile(load("g6_realrec")["known_bits"], -(-K * mu // 4096))
    p = orc.RxParams(N=4096, CP=224, P=2, D=D, lo=100, hi=100 + C, const_points=pts, const_bits=np.asarray(bt).astype(np.int64), known_bits=known)
    eng = engine_for(p)
    F = 5
    rs = np.random.RandomState(C)
    bits = rs.randint(0, 2, (F, D * C * mu)).astype(np.uint8)
    packed = torch.from_numpy(np.stack([np.packbits(b) for b in bits])).cuda()
    assert packed.shape[1] == eng.bytes_per_frame
    mask = known[: C * mu]
    want_plain = bits.reshape(-1).astype(np.int64)
    want_xor = want_plain ^ np.resize(mask, want_plain.shape).astype(np.int64)
    for m, want in ((None, want_plain), (mask, want_xor)):
        dev = eng.unpack_decode(packed, m, to_host=False)
        host = eng.unpack_decode(packed, m, to_host=True)
        torch.cuda.synchronize()
        assert dev.dtype == torch.int64 and np.array_equal(dev.cpu().numpy(), want)
        assert not host.is_cuda and host.is_pinned() and np.array_equal(host.numpy(), want)
    pageable = np.zeros(want_plain.size + 2, dtype=np.int64)
    addr = pageable.ctypes.data + (-pageable.ctypes.data) % 16
    rc = eng.lib.gf3_unpack_bits(eng._h, ctypes.c_void_p(packed.data_ptr()), F, None, 0, ctypes.c_void_p(addr), None)
    assert rc == -1 and b"pinned" in eng.lib.gf3_last_error(None)


def test_receive_host_list_exactly_full_and_read_only_mapping(tmp_path):
    """ (i) a kept-lag list that is EXACTLY full when a piece begins: the piece is offered no room (cap 0, no
    buffers) and is either empty or overflows into the second look -- for every capacity from 1 to the number of lags
    the stream keeps, the detections and bits are the oracle's; (ii) a read-only file mapping as the source."""
    g = load("g1_n1024_qpsk")
    p = params_of(g)
    r, payload = _crafted_stream(p, 50)
    ref = orc.receive(r, p)
    want_peaks = np.flatnonzero(ref["zeros"])
    eng = engine_for(p)
    base = eng.receive_host(r, chunk_samples=1)
    listed = base["info"]["listed"]
    assert 4 <= listed <= 400, base["info"]
    # the calling thread's cached piece buffers and kept-lag list are large enough for every call below: the same
    # device memory serves them all, handed out as slices
    cached = lambda: {k: eng._tls.ingest.tensors[k].data_ptr() for k in ("buf0", "buf1", "list idx", "list val")}
    ptrs = cached()
    full = 0
    for cap in range(1, listed + 1):
        out = eng.receive_host(r, chunk_samples=1, list_cap=cap)
        full += out["info"]["full_list_pieces"]
        assert np.array_equal(out["peaks"].cpu().numpy(), want_peaks), (cap, out["info"])
        assert torch.equal(out["bits"], base["bits"]), cap
        assert cached() == ptrs, cap
    assert full >= 1                                                    # some capacity left a piece no room at all
    assert np.array_equal(eng.unpack_bits(base["bits"]).cpu().numpy(), ref["bits"])
    # (ii) a read-only file mapping is taken like any other pageable array (staged: host copies two pieces ahead, on a
    #      background thread), and nothing is left behind for the next launch check
    path = tmp_path / "stream.f64"
    r.tofile(path)
    ro = np.memmap(path, dtype=np.float64, mode="r")
    out = eng.receive_host(ro, chunk_samples=1)
    assert out["info"]["source"] == "pageable, staged" and out["info"]["chunks"] >= 4 and not out["info"]["pinned_input"], out["info"]
    assert np.array_equal(out["peaks"].cpu().numpy(), want_peaks) and torch.equal(out["bits"], base["bits"])
    del ro
    assert eng.lib.gf3_clear_runtime_error() == 0
    assert torch.equal(eng.sync_stream(torch.from_numpy(r).cuda()), out["peaks"])


def test_receive_host_large_pageable_stream_is_copied_by_the_runtime():
    """The default for pageable memory: a stream of 128 MiB or more is cut into equal pieces of at least 128 MiB and each
    piece is handed to the runtime as it is (which pins a source of that size on the fly); smaller streams are staged.
    1 400 config-3 packets (439 MB of f32): three pieces, the peaks and bits of the one-shot path, every sample over
    PCIe once."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("config3_tool", os.path.join(os.path.dirname(__file__), "..", "tools", "config3.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    eng, cfg, channel = tool.make_engine()
    r, payload = tool.make_stream(eng, channel, 1400, seed=13)
    host = r.cpu().numpy().copy()
    out = eng.receive_host(host)
    info = out["info"]
    assert info["source"].startswith("pageable, copied by the runtime") and info["chunks"] == 3 and not info["pinned_input"], info
    assert info["chunk_samples"] * 4 >= (128 << 20) and info["h2d_bytes"] == host.nbytes, info
    one = eng.sync_stream(r)
    assert torch.equal(out["peaks"], one) and one.numel() == 1401
    assert torch.equal(out["bits"], eng.demod_frames(r, (one + 2)[:-1])["bits"])
    single = eng.receive_host(host[: 64 + 800 * cfg.frame_len + cfg.chirp_length + 200].copy())      # 251 MB: one piece, the runtime's
    assert single["info"]["source"].startswith("pageable, copied by the runtime") and single["info"]["chunks"] == 1, single["info"]
    assert torch.equal(single["peaks"], one[:801]) and torch.equal(single["bits"], out["bits"][:800])
    staged = eng.receive_host(host[: 64 + 300 * cfg.frame_len + cfg.chirp_length + 200].copy())      # 94 MB: staged
    assert staged["info"]["source"] == "pageable, staged" and torch.equal(staged["peaks"], one[:301]), staged["info"]


# ---------------------------------------------------------------------------------------------------------------
# the screened frames-mode sync (gf3_sync_frames_ex mode 1; gf3rx_fscreen.h)
# ---------------------------------------------------------------------------------------------------------------
def _window_lags_fp64(r, p, s0, W):
    """y[j] = sum_k r[s0 + j + k] c[k], j < W, in fp64 (samples beyond the stream are zeros)"""
    c = orc.chirp_replica(p)
    seg = np.zeros(W + p.Lc - 1)
    lo, hi = max(0, s0), min(len(r), s0 + len(seg))
    if hi > lo:
        seg[lo - s0: hi - s0] = r[lo:hi]
    return np.correlate(seg, c, mode="valid")


@pytest.mark.parametrize("N,CP,mu,dt", [(1024, 128, 2, torch.float32), (4096, 512, 2, torch.float32), (2048, 256, 6, torch.float64),
                                        (4096, 224, 2, torch.int16), (8192, 1024, 2, torch.float32)])
def test_screened_sync_frames_equals_fp64_and_bound_holds(N, CP, mu, dt):
    """Every window of a batch through the fp32 screen: (i) the bound E covers |y32 - y| for every lag of every window, against
    fp64 dot products on the host (clean windows, noisy ones, a window hanging over the end of the buffer, an empty one);
    (ii) the screened call returns exactly the all-fp64 kernel's indices; (iii) clean windows are resolved by the screen
    alone, and only unresolved ones reach the fp64 kernel."""
    pts, bt = orc.qpsk_table() if mu == 2 else orc.square_qam_table(mu)
    K = N // 2 - 1
    known = load("g6_realrec")["known_bits"]
    known = np.tile(known, -(-K * mu // len(known)))
    p = orc.RxParams(N=N, CP=CP, P=2, D=2, lo=1, hi=K, const_points=pts, const_bits=bt, known_bits=known,
                     fit_lo=min(500, K // 2), fit_hi=min(1000, K))
    F = 8
    rows, gaps, payload = _rows_with_gaps(p, F, seed=3 * N + mu)
    rs = np.random.RandomState(N)
    rows[2] += 0.05 * rs.randn(rows.shape[1])                  # a noisy window
    rows[3] += 0.6 * rs.randn(rows.shape[1])                   # chirp near the noise: extrema everywhere around the threshold
    rows[5] = 1e-3 * rs.randn(rows.shape[1])                   # no chirp at all
    rows[6] = 0.0                                              # silence: the maximum is not above zero
    rows[5, -64:] = 0.0                                        # (window 6 starts 8 samples inside row 5)
    if dt == torch.int16:
        q = np.round(rows * (20000.0 / np.abs(rows).max()))
        x = torch.from_numpy(q.astype(np.int16)).cuda(); r64 = q.reshape(-1)
    elif dt == torch.float32:
        x = torch.from_numpy(rows.astype(np.float32)).cuda(); r64 = rows.astype(np.float32).astype(np.float64).reshape(-1)
    else:
        x = torch.from_numpy(rows).cuda(); r64 = rows.reshape(-1)
    eng = engine_for(p, in_dtype=dt, max_window=320)
    stride, lo, W = rows.shape[1], -8, 320
    d = eng.debug_frames_screen(x, F, stride, lo, lo + W)
    y32, err, cls = d["y32"].cpu().numpy(), d["err"].cpu().numpy(), d["cls"].cpu().numpy()
    worst = 0.0
    for f in range(F):
        y = _window_lags_fp64(r64, p, f * stride + lo, W)
        e = np.abs(y32[f].astype(np.float64) - y).max()
        assert e <= err[f], (f, e, err[f])
        worst = max(worst, e / err[f])
    assert worst < 0.5, worst                                  # (the constant is generous: realised / bound stays far below 1)
    ref = eng.sync_frames(x, F, stride, lo, lo + W)
    scr = eng.sync_frames(x, F, stride, lo, lo + W, screened=True)
    assert torch.equal(ref, scr)
    clean = [0, 1, 4, 7]
    assert all(cls[f] == 0 for f in clean), cls              # decided by the screen alone ...
    assert np.array_equal(d["starts"].cpu().numpy()[clean], ref.cpu().numpy()[clean])   # ... to the fp64 kernel's index
    assert cls[6] == 2, cls                                    # silence: nothing above zero, left to the fp64 kernel (-1)
    assert int(ref[6]) == -1
    assert np.array_equal(np.flatnonzero(cls == 2), d["unresolved"].cpu().numpy())
    assert (cls == 2).sum() < F                                # (the screen is selective here)


def test_screened_sync_frames_on_multipath_and_narrow_windows():
    """The multipath fixture (echoes: several extrema above the threshold before the largest): screened == fp64 for windows
    narrower than the plan's, starting at odd offsets, and for a window wider than the plan (the call then IS the fp64 one)."""
    g = load("g3_n4096_16qam_gr5")
    p = params_of(g)
    eng = engine_for(p, max_window=400)
    x = torch.from_numpy(g["r"]).cuda()
    for pk in g["peaks"][:-1]:
        s_true = int(pk) + 1 - (p.Lc - 1)
        for lo, W in ((s_true - 150, 400), (s_true - 33, 97), (s_true - 5, 11), (s_true - 299, 300), (s_true + 3, 50)):
            a = eng.sync_frames(x, 1, 0, lo, lo + W)
            b = eng.sync_frames(x, 1, 0, lo, lo + W, screened=True)
            assert torch.equal(a, b), (lo, W, a, b)
    eng2 = engine_for(p, max_window=1400)                      # wider than the screen's transform allows: no plan, fp64 either way
    lo = int(g["peaks"][0]) + 1 - (p.Lc - 1) - 600
    assert torch.equal(eng2.sync_frames(x, 1, 0, lo, lo + 1400), eng2.sync_frames(x, 1, 0, lo, lo + 1400, screened=True))


def test_screened_sync_frames_full_size_round_trip():
    """BASELINE config-2 geometry, 4 096 distinct packets with jitter gaps: the screened sync returns every offset, none of
    the windows needs the fp64 kernel, and the demodulated payload is exact."""
    pts, bt = orc.qpsk_table()
    K = 2047
    known = np.tile(load("g6_realrec")["known_bits"], -(-K * 2 // 4096))
    p = orc.RxParams(N=4096, CP=512, P=2, D=8, lo=1, hi=K, const_points=pts, const_bits=bt, known_bits=known)
    eng = engine_for(p, in_dtype=torch.float32, max_window=320)
    F, stride = 4096, 78720
    gen = torch.Generator(device="cuda").manual_seed(11)
    packed = torch.randint(0, 256, (F, eng.bytes_per_frame), dtype=torch.uint8, device="cuda", generator=gen)
    gaps = torch.randint(0, 300, (F,), dtype=torch.int64, device="cuda", generator=gen)
    filler = np.zeros(K, dtype=complex); filler[K - 1] = (1 - 1j) / np.sqrt(2)
    rows = eng.tx_frames(packed, filler, stride=stride, gaps=gaps, out_dtype=torch.float32)
    work = eng.sync_frames_workspace(F)
    starts = eng.sync_frames(rows, F, stride, -8, 312, screened=True, work=work)
    assert torch.equal(starts, torch.arange(F, device="cuda") * stride + gaps + p.Lc)
    assert int(work[:4].view(torch.int32).item()) == 0         # every window decided by the screen
    assert torch.equal(eng.demod_frames(rows, starts)["bits"], packed)
    assert torch.equal(starts, eng.sync_frames(rows, F, stride, -8, 312))
