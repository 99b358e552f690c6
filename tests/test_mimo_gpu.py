"""2 x 2 spatial multiplexing on the GPU: gf3_mimo_pilots and gf3_mimo_detect against the NumPy restatement
(tests/mimo_ref.py), the cover identity against the demodulator's own estimates, the single-stream limit against
gf3_combine_branches, edge inputs and argument checks, and transmit_mimo -> the scenario's room -> receive_mimo end to end
(tests/test_mimo_cpu.py holds the CPU form and settles the coded level).  The guard-band rows of the two entries are in
tests/test_bounds_mimo_gpu.py.

Shapes: N = 1024, CP in {0, 64}, P in {2, 4}, D = 7, data bins 5 .. 399 (C = 395: two 256-carrier tiles, the second
partial), F = 3."""
import contextlib
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import mimo_ref as MR
from tests import tables as T
from tests.joint_checks import held_to_the_restatement
from tests.test_mimo_cpu import LEVEL_DB

pytestmark = pytest.mark.gpu
F3 = 3


def engine_of(p, **kw):
    from gf3_audio_modem_amd import Engine, RxConfig
    return Engine(RxConfig(N=p.N, CP=p.CP, P=p.P, D=p.D, data_bins=p.data_carriers, const_points=p.const_points,
                           const_bits=p.const_bits, known_bits=p.known_bits, in_dtype=torch.float64,
                           fit_lo=p.fit_lo, fit_hi=p.fit_hi, **kw))


def small_params(CP=64, P=2, table=None, carriers=None, D=7, N=1024):
    pts, bits = orc.qpsk_table() if table is None else table
    bits = np.asarray(bits).astype(np.int64)
    known = np.random.default_rng(99).integers(0, 2, size=(N // 2 - 1) * bits.shape[1]).astype(np.uint8)
    return orc.RxParams(N=N, CP=CP, P=P, D=D, lo=5, hi=400, carriers=carriers, const_points=np.asarray(pts), const_bits=bits,
                        known_bits=known, fit_lo=10, fit_hi=300)


def same_bytes(a, b):
    return np.array_equal(a.cpu().numpy().reshape(-1).view(np.uint8), b.cpu().numpy().reshape(-1).view(np.uint8))


# ---- gf3_mimo_pilots ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pilot_case(CP, P):
    """Three packet pairs through the scenario's room with a little noise, microphone 0 -> (p, samples, starts)"""
    p = small_params(CP, P)
    rng = np.random.default_rng(CP + P)
    bits = rng.integers(0, 2, size=2 * F3 * p.D * p.C * p.mu)
    tx2 = MR.tx_mimo(bits, rng.choice(T.QPSK_FILL, size=p.K - p.C), p, lead=100, tail=300)
    r = MR.through(tx2)[0]
    r = r + 0.01 * np.sqrt(np.mean(r * r)) * rng.normal(size=len(r))
    starts = 100 + np.arange(F3) * p.frame_len + p.Lc + MR.LEAD - (16 if CP else 0)
    return p, r, starts.astype(np.int64)


@pytest.mark.parametrize("CP", [0, 64])
@pytest.mark.parametrize("P", [2, 4])
def test_pilots_against_the_restatement(CP, P):
    p, r, starts = pilot_case(CP, P)
    eng = engine_of(p)
    H, status = eng.mimo_pilots(r, starts)
    ref, ref_status = MR.pilots(r, starts, p)
    got = H.cpu().numpy()
    assert got.dtype == np.complex128 and got.shape == (F3, 2, 2, p.K) and status.dtype == torch.int32
    assert status.cpu().numpy().tolist() == ref_status.tolist() == [0, 0, 0]
    print(f"CP {CP}, P {P}: worst relative deviation from the restatement {np.abs(got / ref - 1).max():.2e}")
    np.testing.assert_allclose(got, ref, rtol=1e-12)
    # cover 0 is the demodulator's own estimate
    o = eng.demod_frames(r, starts, want=("Hs", "He"))
    print(f"CP {CP}, P {P}: cover 0 against demod_frames {np.abs(got[:, 0, 0] / o['Hs'].cpu().numpy() - 1).max():.2e}")
    np.testing.assert_allclose(got[:, 0, 0], o["Hs"].cpu().numpy(), rtol=1e-11)
    np.testing.assert_allclose(got[:, 1, 0], o["He"].cpu().numpy(), rtol=1e-11)
    H2, status2 = eng.mimo_pilots(r, starts)
    assert same_bytes(H, H2) and same_bytes(status, status2)
    # a packet cut off at either end: status 1 and NaN rows, the neighbours as they were
    L = p.M * p.S
    off = np.array([-1, starts[0], len(r) - L + 1, starts[1], len(r), starts[2], -2 ** 40, 2 ** 40], dtype=np.int64)
    Hc, sc = eng.mimo_pilots(r, off)
    Hc = Hc.cpu().numpy()
    assert sc.cpu().numpy().tolist() == [1, 0, 1, 0, 1, 0, 1, 1]
    assert np.isnan(Hc[[0, 2, 4, 6, 7]].real).all() and np.isnan(Hc[[0, 2, 4, 6, 7]].imag).all()
    assert np.array_equal(Hc[[1, 3, 5]], got)
    # the last packet ending on the last sample
    He_, se = eng.mimo_pilots(r[: starts[2] + L], starts)
    assert se.cpu().numpy().tolist() == [0, 0, 0] and np.array_equal(He_.cpu().numpy(), got)


@pytest.mark.parametrize("N", [2048, 4096, 8192])
def test_pilots_at_the_other_transform_sizes(N):
    """One packet pair of 2 + 1 + 2 symbols per size (the kernel is instantiated per transform size), in float32 samples"""
    p = small_params(CP=32, P=2, D=1, N=N)
    rng = np.random.default_rng(N)
    bits = rng.integers(0, 2, size=2 * p.D * p.C * p.mu)
    r = MR.through(MR.tx_mimo(bits, rng.choice(T.QPSK_FILL, size=p.K - p.C), p, lead=10, tail=100))[1].astype(np.float32)
    starts = np.array([10 + p.Lc + MR.LEAD - 8])
    from gf3_audio_modem_amd import Engine, RxConfig
    eng = Engine(RxConfig(N=p.N, CP=p.CP, P=p.P, D=p.D, data_bins=p.data_carriers, const_points=p.const_points, const_bits=p.const_bits,
                          known_bits=p.known_bits, in_dtype=torch.float32, fit_lo=p.fit_lo, fit_hi=p.fit_hi))
    H, status = eng.mimo_pilots(r, starts)
    ref, _ = MR.pilots(r, starts, p)
    assert status.cpu().numpy().tolist() == [0]
    np.testing.assert_allclose(H.cpu().numpy(), ref, rtol=1e-12)


def test_pilots_refusals():
    p = small_params(P=3)
    eng = engine_of(p)
    with pytest.raises(ValueError, match="gf3_mimo_pilots.*even"):
        eng.mimo_pilots(np.zeros(40000), [0])
    eng = engine_of(small_params(P=1))
    with pytest.raises(ValueError, match="gf3_mimo_pilots"):
        eng.mimo_pilots(np.zeros(40000), [0])
    eng = engine_of(small_params(P=2))
    H, status = eng.mimo_pilots(np.zeros(40000), np.zeros(0, dtype=np.int64))
    assert H.shape == (0, 2, 2, 511) and status.numel() == 0


# ---- gf3_mimo_detect ---------------------------------------------------------------------------------------------------
def detect_inputs(p, F, B, seed):
    """Random spectra [F*D, N/2+1], estimates [F, 2, 2, K] whose end block differs from the start block in magnitude and
    phase, slopes [F] of a few 1e-3 rad per carrier"""
    rng = np.random.default_rng(seed)
    cn = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    Ys = [cn(F * p.D, p.N // 2 + 1) for _ in range(B)]
    Hs = []
    for _ in range(B):
        H = cn(F, 2, 2, p.K) * 0.7
        H[:, 1] = H[:, 0] * (1 + 0.3 * rng.normal(size=(F, 2, p.K))) * np.exp(0.2j * rng.normal(size=(F, 2, p.K)))
        Hs.append(H)
    slopes = [3e-3 * rng.normal(size=F) for _ in range(B)]
    return Ys, Hs, slopes


def check_detect(p, eng, Ys, Hs, slopes, packets=None):
    """One call against the restatement (on `packets` alone where given), the signs against its joint argmin, a second
    call's bytes -> the LLRs"""
    llr = eng.mimo_detect(Ys, Hs, slopes)
    got = llr.cpu().numpy()
    F = np.asarray(Hs[0]).shape[0]
    assert got.dtype == np.float32 and got.shape == (F, 2, p.D, p.C, 2)
    assert same_bytes(llr, eng.mimo_detect(Ys, Hs, slopes))
    part = got
    if packets is not None:
        rows = (np.asarray(packets)[:, None] * p.D + np.arange(p.D)).reshape(-1)
        Ys, Hs, slopes = [y[rows] for y in Ys], [h[packets] for h in Hs], [s[packets] for s in slopes]
        part = got[packets]
    ref, pair = MR.detect(Ys, Hs, slopes, p)
    held_to_the_restatement(part, ref, pair, p.const_bits)
    return got


@pytest.mark.parametrize("kind,P", [("qpsk", 2), ("qpsk", 4), ("qam4_binary", 2), ("shuffled", 4), ("qpsk_rot", 2)])
def test_detect_against_the_restatement(kind, P):
    """B = 1 .. 4 with the reference's QPSK, the binary-indexed 4-QAM, a 4-point table that is no grid, and on a scattered
    carrier map (Y and the estimates are read through the carriers' bins)."""
    table = {"qam4_binary": orc.square_qam_table(2), "qpsk_rot": T.TABLES["qpsk_rot"]}.get(kind)
    p = small_params(P=P, table=table, carriers=T.MAPS["shuffled"](511) if kind == "shuffled" else None)
    eng = engine_of(p)
    Ys, Hs, slopes = detect_inputs(p, F3, 4, len(kind) + P)
    for B in (1, 2, 3, 4):
        check_detect(p, eng, Ys[:B], Hs[:B], slopes[:B])


def test_detect_runs_of_symbols_per_workgroup():
    """64 packet pairs of 96 symbols on 257 carriers: a workgroup then takes a run of consecutive symbols (6 on 256
    compute units) and advances its phasors from symbol to symbol; three packets are held to the restatement."""
    p = small_params(P=2, D=96, carriers=np.arange(5, 262))
    eng = engine_of(p)
    Ys, Hs, slopes = detect_inputs(p, 64, 2, 61)
    check_detect(p, eng, Ys, Hs, slopes, packets=[0, 37, 63])


def test_detect_edge_inputs():
    p = small_params()
    eng = engine_of(p)
    Ys, Hs, slopes = detect_inputs(p, F3, 2, 21)
    Ys, Hs = [y.copy() for y in Ys], [h.copy() for h in Hs]
    bins = p.data_carriers
    cell = lambda f, l: f * p.D + l
    Ys[0][cell(0, 3), bins[17]] = complex(np.nan, 0.0)     # one branch's y: the other decides alone
    Ys[1][cell(1, 4), bins[300]] = complex(1.0, np.inf)
    Hs[0][2, 1, 1, bins[40] - 1] = complex(0.0, np.nan)    # one estimate of one branch: that carrier of that packet, every symbol
    Hs[1][0, 0, 0, bins[41] - 1] = complex(np.inf, 0.0)
    for y in Ys:                                           # every branch: nothing is left
        y[cell(1, 5), bins[258]] = complex(np.nan, np.nan)
    Ys[0][cell(2, 6), bins[2]], Hs[1][2, 0, 1, bins[2] - 1] = complex(0.0, -np.inf), complex(np.nan, 1.0)
    got = check_detect(p, eng, Ys, Hs, slopes)
    assert np.isfinite(got).all()
    alone = [eng.mimo_detect([Ys[b]], [Hs[b]], [slopes[b]]).cpu().numpy() for b in range(2)]
    tol = dict(rtol=1e-6, atol=1e-9 * np.abs(got).max())    # (the other branch decides alone: its own one-branch LLRs)
    np.testing.assert_allclose(got[0, :, 3, 17], alone[1][0, :, 3, 17], **tol)
    np.testing.assert_allclose(got[1, :, 4, 300], alone[0][1, :, 4, 300], **tol)
    np.testing.assert_allclose(got[2, :, :, 40], alone[1][2, :, :, 40], **tol)
    np.testing.assert_allclose(got[0, :, :, 41], alone[0][0, :, :, 41], **tol)
    for dead in (got[1, :, 5, 258], got[2, :, 6, 2]):
        assert not dead.any() and not np.signbit(dead).any()
    # every branch dead everywhere: +0, no sign bit
    Hn = [np.full_like(h, complex(np.nan, np.nan)) for h in Hs]
    dead = eng.mimo_detect(Ys, Hn, slopes).cpu().numpy()
    assert not dead.any() and not np.signbit(dead).any()


def test_single_stream_limit_is_the_diversity_combiner():
    """Column 1 exactly zero and Y_b = eq_b Hest_b from the oracle's model: stream 0's LLRs are gf3_combine_branches' on
    (eq_b, Hs_b, He_b) within the float32 tolerance, stream 1's are all +0."""
    p = small_params(P=4)
    eng = engine_of(p)
    rng = np.random.default_rng(31)
    B, F = 3, F3
    idx = rng.integers(0, 4, size=(F * p.D, p.C))
    eqs, Hss, Hes, Ys, Hm, slopes = [], [], [], [], [], []
    for _ in range(B):
        eq = p.const_points[idx] + (rng.normal(size=idx.shape) + 1j * rng.normal(size=idx.shape)) * 0.1
        Hs = (rng.normal(size=(F, p.K)) + 1j * rng.normal(size=(F, p.K))) * 0.7
        He = Hs * (1 + 0.3 * rng.normal(size=(F, p.K))) * np.exp(0.2j * rng.normal(size=(F, p.K)))
        slope = 3e-3 * rng.normal(size=F)
        Hest = orc.channel_model(Hs, He, slope, p)[:, :, p.data_carriers - 1].reshape(F * p.D, p.C)
        Y = np.zeros((F * p.D, p.N // 2 + 1), dtype=complex)
        Y[:, p.data_carriers] = eq * Hest
        H = np.zeros((F, 2, 2, p.K), dtype=complex)
        H[:, 0, 0], H[:, 1, 0] = Hs, He
        eqs.append(eq); Hss.append(Hs); Hes.append(He); Ys.append(Y); Hm.append(H); slopes.append(slope)
    for n in (1, 3):
        got = eng.mimo_detect(Ys[:n], Hm[:n], slopes[:n]).cpu().numpy()
        ref = eng.combine_branches(eqs[:n], Hs=Hss[:n], He=Hes[:n], want=("llr",))["llr"].cpu().numpy().reshape(F, p.D, p.C, 2)
        np.testing.assert_allclose(got[:, 0], ref, rtol=1e-6, atol=1e-9 * np.abs(ref).max())
        assert not got[:, 1].any() and not np.signbit(got[:, 1]).any()


def test_detect_argument_checks():
    from gf3_audio_modem_amd import _lib
    p = small_params()
    eng = engine_of(p)
    F = 2
    Ys, Hs, slopes = detect_inputs(p, F, 2, 8)
    n = F * 2 * p.D * p.C * 2
    bad = [dict(Ys=[]), dict(Ys=Ys * 3, Hs=Hs * 3, slopes=slopes * 3), dict(Hs=Hs[:1]), dict(slopes=slopes * 2),
           dict(Ys=[Ys[0], Ys[1][: p.D]]), dict(Ys=[y[:-1] for y in Ys]), dict(Hs=[Hs[0], Hs[1][:1]]), dict(slopes=[slopes[0], slopes[1][:1]]),
           dict(out=torch.empty(n - 1, dtype=torch.float32, device="cuda")), dict(out=torch.empty(n, dtype=torch.float64, device="cuda")),
           dict(out=torch.empty(2 * n, dtype=torch.float32, device="cuda")[::2])]
    for kw in bad:
        with pytest.raises(ValueError, match="mimo_detect"):
            eng.mimo_detect(**{**dict(Ys=Ys, Hs=Hs, slopes=slopes), **kw})
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    o = eng.mimo_detect(Ys, Hs, slopes, out=out)
    assert o.data_ptr() == out.data_ptr() and same_bytes(o, eng.mimo_detect(Ys, Hs, slopes))
    empty = eng.mimo_detect([np.zeros((0, 513), complex)] * 2, [np.zeros((0, 2, 2, 511), complex)] * 2, [np.zeros(0)] * 2)
    assert empty.shape == (0, 2, p.D, p.C, 2)
    # a 16-QAM context: the façade and the library both refuse
    p16 = small_params(table=orc.square_qam_table(4))
    e16 = engine_of(p16)
    with pytest.raises(ValueError, match="mimo_detect.*mu = 2"):
        e16.mimo_detect(Ys, Hs, slopes)
    # the raw ABI
    lib = eng.lib
    dY, dH = [eng._dev(y) for y in Ys], [eng._dev(h) for h in Hs]
    dS = [eng._dev(s, torch.float64) for s in slopes]
    tab = lambda xs: (C.c_void_p * len(xs))(*[None if x is None else x.data_ptr() for x in xs])
    Yt, Ht, St, q = tab(dY), tab(dH), tab(dS), _lib.ptr(out)
    call = lambda *a: lib.gf3_mimo_detect(*a, None)
    assert call(eng._h, 2, Yt, Ht, St, 0, q) == 0 and call(eng._h, 9, None, None, None, 0, None) == 0      # F == 0: a no-op
    cases = {"no context": (None, 2, Yt, Ht, St, F, q), "B = 0": (eng._h, 0, Yt, Ht, St, F, q), "B = 5": (eng._h, 5, Yt, Ht, St, F, q),
             "no spectra": (eng._h, 2, None, Ht, St, F, q), "no estimates": (eng._h, 2, Yt, None, St, F, q),
             "no slopes": (eng._h, 2, Yt, Ht, None, F, q), "null spectrum": (eng._h, 2, tab([dY[0], None]), Ht, St, F, q),
             "null estimate": (eng._h, 2, Yt, tab([None, dH[1]]), St, F, q), "null slope": (eng._h, 2, Yt, Ht, tab([dS[0], None]), F, q),
             "no output": (eng._h, 2, Yt, Ht, St, F, None), "F < 0": (eng._h, 2, Yt, Ht, St, -1, q),
             "too many packets": (eng._h, 2, Yt, Ht, St, 65536, q), "16-QAM": (e16._h, 2, Yt, Ht, St, F, q)}
    for text, args in cases.items():
        assert call(*args) == _lib.GF3_EINVAL, text
        assert b"gf3_mimo_detect" in lib.gf3_last_error(None), text
    pil = lambda *a: lib.gf3_mimo_pilots(*a, None)
    x, off = eng._dev(np.zeros(40000), torch.float64), eng._dev([0, 100], torch.int64)
    Hq, sq = _lib.ptr(dH[0]), _lib.ptr(torch.zeros(2, dtype=torch.int32, device="cuda"))
    assert pil(eng._h, None, 0, None, 0, None, None) == 0
    for text, args in {"no context": (None, _lib.ptr(x), 40000, _lib.ptr(off), 2, Hq, sq), "no samples": (eng._h, None, 40000, _lib.ptr(off), 2, Hq, sq),
                       "no offsets": (eng._h, _lib.ptr(x), 40000, None, 2, Hq, sq), "no output": (eng._h, _lib.ptr(x), 40000, _lib.ptr(off), 2, None, sq),
                       "no status": (eng._h, _lib.ptr(x), 40000, _lib.ptr(off), 2, Hq, None), "F < 0": (eng._h, _lib.ptr(x), 40000, _lib.ptr(off), -1, Hq, sq),
                       "n < 0": (eng._h, _lib.ptr(x), -1, _lib.ptr(off), 2, Hq, sq)}.items():
        assert pil(*args) == _lib.GF3_EINVAL, text
        assert b"gf3_mimo_pilots" in lib.gf3_last_error(None), text
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------------------------------
LEAD, TAIL = 300, 400


def facade(encoding, **attrs):
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A3", encoding=encoding, no_pilots=4, packet_length=4)
    for k, v in attrs.items():
        setattr(rx, k, v)
    return rx


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


@functools.lru_cache(maxsize=None)
def recordings(encoding):
    """One packet pair through transmit_mimo and the scenario's room, noiseless -> (payload, stereo signal, [mic 0, mic 1])"""
    rx = facade(encoding)
    n = 9 * 768 if encoding.startswith("QCLDPC") else 2 * 4 * 1800
    payload = np.random.default_rng(3).integers(0, 2, size=n)
    np.random.seed(5)                                       # (the fill of the last packet, the filler of the unused carriers)
    tx2 = quiet(rx.transmit_mimo, payload)
    assert tx2.dtype == np.float64 and tx2.shape == (2, 2 * rx.chirp_length + 12 * 4320) and rx.no_packets == 2
    tx2 = np.concatenate([np.zeros((2, LEAD)), tx2, np.zeros((2, TAIL))], axis=1)
    return payload, tx2, MR.through(tx2)


def oracle_params(rx):
    pts, bt = orc.qpsk_table()
    return orc.RxParams(N=4096, CP=224, P=4, D=4, lo=100, hi=1000, const_points=pts, const_bits=bt,
                        known_bits=np.asarray(rx.known_sequence, dtype=np.uint8))


def test_transmit_mimo_format():
    """Row 0 is transmit() of the even-numbered packets, bit for bit, when seeded alike; row 1 is silent under every chirp,
    carries the odd-numbered packets' data symbols as transmit() makes them and their pilots under the cover."""
    payload, tx2, _ = recordings("None")
    rx = facade("None")
    nbp = 4 * 1800
    np.random.seed(5)
    even = quiet(rx.transmit, payload[:nbp])
    np.random.seed(5)
    odd = quiet(rx.transmit, payload[nbp:])
    Lc, S = rx.chirp_length, 4320
    body = slice(LEAD + Lc, LEAD + Lc + 12 * S)
    assert np.array_equal(tx2[0, LEAD: LEAD + len(even)], even)
    assert not tx2[1, LEAD: LEAD + Lc].any() and not tx2[1, body.stop:].any()
    want = odd[Lc: Lc + 12 * S].reshape(12, S).copy()
    want[[1, 3, 9, 11]] *= -1.0
    assert np.array_equal(tx2[1, body].reshape(12, S), want)
    # the restatement builds the same two streams from the same bits and filler
    p = oracle_params(rx)
    np.random.seed(5)
    np.random.binomial(n=1, p=0.5, size=(0,))
    fill = rx.random_qpsk()
    ref = MR.tx_mimo(payload, fill, p, lead=LEAD, tail=TAIL)
    assert np.abs(tx2 - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("encoding", ["None", "XOR"])
def test_receive_mimo_noiseless_is_exact(encoding):
    payload, tx2, rec = recordings(encoding)
    rx = facade(encoding)
    bits, Hs0, He0 = quiet(rx.receive_mimo, rec)
    assert bits.dtype == np.int64 and np.array_equal(bits, payload) and rx.no_packets == 1
    # what it publishes, against the restatement on the same samples
    p = oracle_params(rx)
    o = MR.receive_mimo(rec, p)
    assert rx.last_branch_starts.dtype == np.int64 and np.array_equal(rx.last_branch_starts, o["starts"])
    sep = rx.last_mimo_separation
    assert sep.dtype == np.float64 and sep.shape == (1, 900)
    np.testing.assert_allclose(sep, o["separation"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(Hs0, o["H"][0][0, 0, 0], rtol=1e-9, atol=1e-9 * np.abs(Hs0).max())
    np.testing.assert_allclose(He0, o["H"][0][0, 1, 0], rtol=1e-9, atol=1e-9 * np.abs(He0).max())
    assert rx.last_clock_ppm is None and rx.sync_report is None
    # a 2-D array, and three recordings of which one is a copy
    assert np.array_equal(quiet(rx.receive_mimo, np.stack(rec))[0], payload)
    assert np.array_equal(quiet(rx.receive_mimo, rec + [rec[0]])[0], payload)
    assert rx.last_branch_starts.shape == (3, 1)
    if encoding == "None":
        # without the advance speaker 1 falls out of microphone 0's window: the same samples do not come back exact
        bare = facade(encoding, mimo_advance=0)
        wrong = int(np.sum(quiet(bare.receive_mimo, rec)[0] != payload))
        print(f"bit errors with mimo_advance = 0: {wrong} of {len(payload)}")
        with pytest.raises(ValueError, match=r"receive_mimo: the recordings hold different numbers of packets: \[1, 3\]"):
            quiet(rx.receive_mimo, [rec[0], np.concatenate([rec[1], rec[1]])])


def test_receive_mimo_coded_at_the_settled_level():
    payload, tx2, rec = recordings("QCLDPC-1/2")
    rx = facade("QCLDPC-1/2")
    bits, _, _ = quiet(rx.receive_mimo, MR.add_noise(rec, tx2, LEVEL_DB))
    print(f"{LEVEL_DB} dB: report {rx.last_decode_report}, median separation {np.median(rx.last_mimo_separation):.2f}")
    assert rx.last_decode_report["codewords"] == 9 and rx.last_decode_report["inner_failed"] == 0
    assert np.array_equal(bits[: len(payload)], payload)


def test_receive_mimo_with_outer_code_and_crc():
    """The outer code's groups are laid out over the EVEN packet count transmit_mimo sends (1000 message bits need one
    packet, two go out: three groups of 2 + 1 codewords instead of one), which is the count the receiver finds."""
    rx = facade("QCLDPC-1/2", outer_code=(2, 1), codeword_crc=True)
    payload = np.random.default_rng(4).integers(0, 2, size=1000)
    np.random.seed(6)
    tx2 = quiet(rx.transmit_mimo, payload)
    assert rx.no_packets == 2 and rx.outer_layout(2) == (9, 3)
    rec = MR.through(np.concatenate([np.zeros((2, LEAD)), tx2, np.zeros((2, TAIL))], axis=1))
    bits, _, _ = quiet(rx.receive_mimo, rec)
    report = rx.last_decode_report
    assert report["codewords"] == 9 and report["inner_failed"] == 0 and report["groups_failed"] == 0 and report["crc_failed"] == 0
    assert len(bits) == 3 * 2 * (768 - 32) and np.array_equal(bits[:1000], payload) and not bits[1000:].any()


def test_mimo_at_the_sound_cards_own_rate():
    """output_rate on the transmitter converts both rows, input_rate on the receiver every recording: 44.1 kHz on both ends"""
    payload, _, _ = recordings("None")
    rx = facade("None", output_rate=44100.0, input_rate=44100.0)
    np.random.seed(5)
    tx2 = quiet(rx.transmit_mimo, payload)
    n48 = 2 * rx.chirp_length + 12 * 4320
    assert tx2.shape[0] == 2 and abs(tx2.shape[1] - n48 * 44100 / 48000) < 2 and rx.last_tx_report["output_samples"] == tx2.shape[1]
    rec = MR.through(np.concatenate([np.zeros((2, LEAD)), tx2, np.zeros((2, TAIL))], axis=1))
    bits, _, _ = quiet(rx.receive_mimo, rec)
    assert np.array_equal(bits, payload)
    assert np.array_equal(rx.last_input_rate, [44100.0, 44100.0])


def test_receive_mimo_local_sync_rule():
    payload, tx2, rec = recordings("None")
    rx = facade("None", sync_rule="local")
    bits, _, _ = quiet(rx.receive_mimo, rec)
    assert np.array_equal(bits, payload)
    rho = np.asarray(rx.sync_report["rho"])
    assert rho.shape == (2, 2) and (rho > 0.3).all() and rx.sync_report["threshold"] == 0.3


def resampled(x, eps, T=32):
    """x as a sound card records it whose sample j is taken at the time j (1 + eps): a Kaiser-windowed sinc of 2 T taps"""
    t = np.arange(int((len(x) - 1) / (1.0 + eps))) * (1.0 + eps)
    i0 = np.floor(t).astype(np.int64)
    frac = t - i0
    xp = np.concatenate([np.zeros(T), x, np.zeros(T + 1)])
    y = np.zeros(len(t))
    for k in range(-T + 1, T + 1):
        u = k - frac
        y += xp[i0 + k + T] * np.sinc(u) * np.i0(9.0 * np.sqrt(np.maximum(1.0 - (u / T) ** 2, 0.0))) / np.i0(9.0)
    return y


def test_receive_mimo_under_clock_correction():
    """Both recordings taken by a sound card 30 ppm fast; clock_correction = 30.0 resamples every packet of every recording."""
    payload, tx2, rec = recordings("None")
    drifted = [resampled(r, 30e-6) for r in rec]
    rx = facade("None", clock_correction=30.0)
    bits, _, _ = quiet(rx.receive_mimo, drifted)
    assert np.array_equal(bits, payload)
    assert rx.last_clock_ppm.shape == (2,) and (rx.last_clock_ppm == 30.0).all() and rx.last_clock_ppm_packets is None
