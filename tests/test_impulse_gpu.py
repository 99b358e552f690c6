"""Impulse noise on the GPU: gf3_noise_estimate_cs / gf3_soft_demap_nw_cs / gf3_interleave (Engine.noise_estimate2,
soft_demap_nw2, interleave) against the NumPy restatement (tests/impulse_ref.py), their edge inputs, and
`interleave = True` with `llr_weighting = "noise2d"` end to end through the façade on a stream with three clicked symbols.
Tolerances are those of tests/test_noise_gpu.py: variances rtol 1e-12, LLRs rtol 1e-6 and atol 1e-9 x max|ref|.  Measured on
the MI355X on test_carrier_counts and test_every_arm_of_the_estimate (32 cases): variances within 4.4e-16 relative."""
import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import impulse_ref as IR
from tests import ldpc_ref as R
from tests import noise_ref as NR
from tests import tables as T
from tests.test_impulse_cpu import D_SMALL, arm_cases, count_case
from tests.util import engine_for, load, modeA2_params, params_of

pytestmark = pytest.mark.gpu
FIXTURES = ["g2_n4096_qpsk", "g3_n4096_16qam_gr5"]


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def check_against_restatement(eng, eq, p):
    """The whole kernel contract on one eq [F*D, C]; -> (var_c, var_s, llr in transmitted order), NumPy."""
    eq_t = torch.as_tensor(eq).cuda()
    eq = _np(eq_t)
    F = eq.shape[0] // p.D
    var_c, var_s = eng.noise_estimate2(eq_t)
    again_c, again_s = eng.noise_estimate2(eq_t)
    assert var_c.dtype == var_s.dtype == torch.float64 and tuple(var_c.shape) == (F, p.C) and tuple(var_s.shape) == (F, p.D)
    assert np.array_equal(_bits(_np(var_c)), _bits(_np(eng.noise_estimate(eq_t))))          # bit-identical to the 1-D estimate
    assert np.array_equal(_bits(_np(var_c)), _bits(_np(again_c))) and np.array_equal(_bits(_np(var_s)), _bits(_np(again_s)))
    ref_c, ref_s = IR.noise_estimate2(eq, p.const_points, p.D)
    fin = np.isfinite(ref_s)
    assert np.array_equal(np.isfinite(_np(var_s)), fin)
    np.testing.assert_allclose(_np(var_s)[fin], ref_s[fin], rtol=1e-12, atol=0)
    llr = _np(eng.soft_demap_nw2(eq_t, var_c, var_s))
    ref = IR.soft_demap_nw2(eq, _np(var_c), _np(var_s), p.const_points, p.const_bits)
    assert llr.dtype == np.float32 and llr.shape == ref.shape == (eq.size * p.mu,)
    assert np.isfinite(llr).all()
    np.testing.assert_allclose(llr, ref, rtol=1e-6, atol=1e-9 * np.abs(ref).max())
    assert np.array_equal(_bits(llr), _bits(_np(eng.soft_demap_nw2(eq_t, var_c, var_s))))
    # de-interleaved in the demapper == the bare permutation of the transmitted order, and both == the restatement's
    fused = _np(eng.soft_demap_nw2(eq_t, var_c, var_s, deinterleave=True))
    two = _np(eng.interleave(torch.from_numpy(llr).cuda(), inverse=True))
    assert np.array_equal(_bits(fused), _bits(two))
    nbp = p.D * p.C * p.mu
    assert np.array_equal(_bits(two.reshape(F, nbp)), _bits(IR.deinterleave(llr.reshape(F, nbp), p.D, p.C, p.mu)))
    return _np(var_c), _np(var_s), llr


def check_interleaver(eng, p, F=3):
    nbp = p.D * p.C * p.mu
    rng = np.random.default_rng(nbp)
    for x in (rng.integers(0, 256, size=(F, nbp), dtype=np.uint8), rng.normal(size=F * nbp).astype(np.float32)):
        y = eng.interleave(x)
        assert y.dtype == torch.as_tensor(x).dtype and tuple(y.shape) == x.shape
        assert np.array_equal(_np(y).reshape(F, nbp), IR.interleave(x.reshape(F, nbp), p.D, p.C, p.mu))
        assert np.array_equal(_np(eng.interleave(y, inverse=True)), x)
        assert np.array_equal(_np(eng.interleave(eng.interleave(x, inverse=True))), x)


@pytest.mark.parametrize("name", FIXTURES)
def test_kernels_match_the_restatement_on_demodulated_streams(name):
    from tests.test_noise_gpu import noisy_eq
    p, eng, eq = noisy_eq(name)
    var_c, var_s, _ = check_against_restatement(eng, eq, p)
    assert var_s.min() > 0
    # a planted profile: one symbol 9 times as noisy -> its LLRs shrink by exactly that factor
    v2 = var_s.copy()
    v2[:, 1] *= 9.0
    l1 = _np(eng.soft_demap_nw2(eq, var_c, var_s)).reshape(-1, p.D, p.C * p.mu)
    l2 = _np(eng.soft_demap_nw2(eq, var_c, v2)).reshape(-1, p.D, p.C * p.mu)
    np.testing.assert_allclose(l2[:, 1], l1[:, 1] / 9.0, rtol=1e-6)
    assert np.array_equal(np.delete(l2, 1, axis=1), np.delete(l1, 1, axis=1))
    check_interleaver(eng, p)


@pytest.mark.parametrize("kind", ["qam64", "qam16_reversed_labels", "ring8", "modeA2_qpsk", "wide_qam64"])
def test_other_tables_and_geometries(kind):
    """64-QAM takes the widest grid kernel; reversed labels and a table that is no grid take the table-generic fall-back
    (mu = 4 and an odd mu = 3); mode A2's geometry (C = 1400: 11 columns per half, a partial last column, s = 2801) with
    QPSK is what the façade runs; 64-QAM on 2046 carriers fills all 16 columns of each half and has index products i s
    beyond 2^32 (in mode A2 they stay below 2^31)."""
    if kind in ("qam64", "wide_qam64"):
        pts, bits = orc.square_qam_table(6)
    elif kind == "qam16_reversed_labels":
        pts, bits = orc.square_qam_table(4)
        bits = bits[:, ::-1].copy()
    elif kind == "ring8":
        pts = np.exp(2j * np.pi * (np.arange(8) + 0.25) / 8) * (1.0 + 0.3 * (np.arange(8) % 2))
        bits = (np.arange(8)[:, None] >> np.arange(2, -1, -1)) & 1
    else:
        pts, bits = orc.qpsk_table()
    bits = np.asarray(bits).astype(np.int64)
    mu = bits.shape[1]
    if kind == "modeA2_qpsk":
        p = modeA2_params(np.zeros(4094, dtype=np.uint8))
        F = 2
    elif kind == "wide_qam64":
        p = orc.RxParams(N=4096, CP=0, P=1, D=60, lo=1, hi=2047, const_points=pts, const_bits=bits,
                         known_bits=np.zeros(2047 * mu, np.uint8), fit_lo=500, fit_hi=1000)
        F = 2
    else:
        p = orc.RxParams(N=1024, CP=0, P=1, D=7, lo=5, hi=400, const_points=pts, const_bits=bits,
                         known_bits=np.zeros(511 * mu, np.uint8), fit_lo=10, fit_hi=100)
        F = 5
    eng = engine_for(p)
    rng = np.random.default_rng(mu)
    idx = rng.integers(0, len(pts), size=(F * p.D, p.C))
    sig = (0.02 + 0.1 * rng.random(p.C)) * (1.0 + 3.0 * (rng.random((F * p.D, 1)) < 0.2))
    eq = pts[idx] + (rng.normal(size=idx.shape) + 1j * rng.normal(size=idx.shape)) * sig
    _, _, llr = check_against_restatement(eng, eq, p)
    check_interleaver(eng, p, F=2)
    if kind == "modeA2_qpsk":
        nbp = p.D * p.C * p.mu
        assert IR.stride(p.C * p.mu, nbp) == 2801
    if kind == "wide_qam64":
        nbp = p.D * p.C * p.mu
        assert p.C == 2046 and (nbp - 1) * IR.stride(p.C * p.mu, nbp) > 2 ** 32
    eng.close()


@pytest.mark.parametrize("table,mp", [("psk8", "descending"), ("rect8", "comb2")])
def test_scattered_carrier_maps(table, mp):
    """The kernels take [F*D, C] and do not care which bins the columns are; tests/tables.py's non-grid tables on a
    descending map and on a comb."""
    i = [k for k, c in enumerate(T.CASES) if c[0] == table and c[1] == mp][0]
    p, x, starts, ref, payload = T.demod_case(i)
    eng = engine_for(p, in_dtype=getattr(torch, T.CASES[i][6]))
    o = eng.demod_frames(torch.from_numpy(x).cuda(), starts, want=("eq",))
    check_against_restatement(eng, o["eq"], p)
    check_interleaver(eng, p, F=2)
    eng.close()


# ---- every noise_estimate_cs_kernel<HI, NCG>, and the carrier counts at which the choice of NCG turns -----------------
def _count_case(table, C, scattered=False):
    p, eq = count_case(table, C, scattered)
    eng = engine_for(p)
    var_c, var_s, llr = check_against_restatement(eng, eq, p)          # (both deinterleave settings)
    ref_c, ref_s = IR.noise_estimate2(eq, p.const_points, p.D)
    print(f"{table} C {C} N {p.N}{' scattered' if scattered else ''}: var_c, var_s against the restatement "
          f"{np.abs(var_c / ref_c - 1).max():.1e} {np.abs(var_s / ref_s - 1).max():.1e} (1e-12)")
    np.testing.assert_allclose(var_c, ref_c, rtol=1e-12, atol=0)
    assert var_c.min() > 0 and var_s.min() > 0 and llr.any()
    eng.close()


@pytest.mark.parametrize("C", [1, 64, 65, 129, 512, 513, 1024, 1025, 1536, 1537, 2047, 2048])
def test_carrier_counts(C):
    """One carrier, one 64-carrier column and one carrier past it, three columns (the second half holds one: its other
    slots lie beyond the half), and both sides of every step of NCG (4 | 8 at 512 | 513, 8 | 12 at 1024 | 1025, 12 | 16 at
    1536 | 1537), every carrier of N = 4096, and the largest accepted count, 2048 (N = 8192: 128 KiB of LDS).  QPSK, D = 3,
    F = 2, the top C bins."""
    _count_case("qpsk_ref", C)


@pytest.mark.parametrize("table,C,scattered", arm_cases())
def test_every_arm_of_the_estimate(table, C, scattered):
    """ring8 and the reference's QPSK (HI = 0: literal scan, per-axis scan), the binary-indexed 4-point grid, square 16-QAM
    and 64-QAM (HI = 1, 2, 3), each at C = 65, 513, 1025 and 1537 (NCG = 4, 8, 12, 16): the sixteen
    noise_estimate_cs_kernel<HI, NCG> and the demapper behind them, five cases on carriers drawn at random
    (tests/test_impulse_cpu.py asserts the census)."""
    _count_case(table, C, scattered)


def test_one_carrier_too_many_is_refused():
    """C = 2049 (N = 8192): gf3_noise_estimate_cs answers GF3_ERANGE and writes nothing."""
    from gf3_audio_modem_amd import _lib
    pts, bits = orc.qpsk_table()
    p = T.params_for((pts, bits), 8192, np.arange(1, 2050), P=1, D=D_SMALL, CP=0)
    eng = engine_for(p)
    eq = torch.from_numpy(pts[np.random.default_rng(1).integers(0, 4, size=(D_SMALL, 2049))]).cuda()
    vc = torch.full((1, 2049), 7.0, dtype=torch.float64, device="cuda")
    vs = torch.full((1, D_SMALL), 7.0, dtype=torch.float64, device="cuda")
    assert eng.lib.gf3_noise_estimate_cs(eng._h, _lib.ptr(eq), 1, _lib.ptr(vc), _lib.ptr(vs), None) == _lib.GF3_ERANGE
    assert b"gf3_noise_estimate_cs" in eng.lib.gf3_last_error(eng._h)
    torch.cuda.synchronize()
    assert (vc == 7.0).all() and (vs == 7.0).all()
    eng.close()


def test_edge_inputs():
    g = load("g2_n4096_qpsk")
    p = params_of(g)
    eng = engine_for(p)
    rng = np.random.default_rng(9)
    F = 4
    idx = rng.integers(0, 4, size=(F * p.D, p.C))
    eq = p.const_points[idx].copy()                                        # packet 0: noiseless (all-zero residual)
    noise = (rng.normal(size=idx.shape) + 1j * rng.normal(size=idx.shape)) * 0.1
    eq[p.D:] += noise[p.D:]
    eq[p.D + 1] = p.const_points[idx[p.D + 1]]                             # packet 1: one symbol without noise (floored)
    eq[2 * p.D + 1, 3] = complex(np.nan, 0.0)                              # packet 2: NaN and Inf samples
    eq[2 * p.D, 8] = complex(np.inf, -1.0)
    var_c, var_s, llr = check_against_restatement(eng, eq, p)              # (packet 3: plain noise)
    assert not var_c[0].any() and not var_s[0].any() and var_s[1, 1] == 0.0
    assert not np.isfinite(var_s[2, [0, 1]]).any() and np.isfinite(var_s[2, 2:]).all()
    assert not np.isfinite(var_c[2, [3, 8]]).any() and np.isfinite(np.delete(var_c[2], [3, 8])).all()
    l4 = llr.reshape(F, p.D, p.C, p.mu)
    plain = NR.maxlog(eq, p.const_points, p.const_bits).reshape(F, p.D, p.C, p.mu)
    np.testing.assert_allclose(l4[0], plain[0], rtol=1e-6)                 # weights 1
    # the NaN / Inf samples erase their symbols and their carriers, and nothing else: the rest of the packet has weight 1
    assert not l4[2][[0, 1]].any() and not l4[2][:, [3, 8]].any()
    keep = np.delete(np.delete(l4[2], [0, 1], axis=0), [3, 8], axis=1)
    np.testing.assert_allclose(keep, np.delete(np.delete(plain[2], [0, 1], axis=0), [3, 8], axis=1), rtol=1e-6)
    vbar = var_c[1].mean()
    np.testing.assert_allclose(l4[1][1], plain[1][1] / (1e-6 * vbar), rtol=1e-6)          # the floor
    # whole packets of zero variance handed in directly, F = 0, a refused F, wrong shapes, bad `out`
    one = torch.as_tensor(eq[:p.D]).cuda()
    z = _np(eng.soft_demap_nw2(one, np.zeros((1, p.C)), np.zeros((1, p.D))))
    np.testing.assert_allclose(z, plain[0].reshape(-1), rtol=1e-6)
    empty = torch.empty((0, p.C), dtype=torch.complex128)
    vc0, vs0 = eng.noise_estimate2(empty)
    assert tuple(vc0.shape) == (0, p.C) and tuple(vs0.shape) == (0, p.D)
    assert eng.soft_demap_nw2(empty, vc0, vs0).numel() == 0 and eng.soft_demap_nw2(empty, vc0, vs0, deinterleave=True).numel() == 0
    assert eng.interleave(torch.empty(0, dtype=torch.float32)).numel() == 0
    out = torch.empty(F * p.D * p.C * p.mu, dtype=torch.float32, device="cuda")
    assert eng.soft_demap_nw2(eq, var_c, var_s, out=out) is out and np.array_equal(_bits(_np(out)), _bits(llr))
    with pytest.raises(ValueError, match="out must be"):
        eng.soft_demap_nw2(eq, var_c, var_s, out=out[:-1])
    with pytest.raises(ValueError, match="eq"):
        eng.noise_estimate2(eq[:-1])
    with pytest.raises(ValueError, match="var_s"):
        eng.soft_demap_nw2(eq, var_c, var_s[:2])
    with pytest.raises(ValueError, match="var_c"):
        eng.soft_demap_nw2(eq, var_c[:2], var_s)
    with pytest.raises(ValueError, match="whole packets"):
        eng.interleave(np.zeros(p.D * p.C * p.mu - 1, dtype=np.uint8))
    with pytest.raises(ValueError, match="uint8 or float32"):
        eng.interleave(np.zeros(p.D * p.C * p.mu, dtype=np.int64))
    from gf3_audio_modem_amd import _lib
    lib = _lib.load()
    d = torch.empty(16, dtype=torch.float64, device="cuda")                # (never touched: every call below is refused)
    ptr = _lib.ptr(d)
    assert lib.gf3_noise_estimate_cs(eng._h, None, 1, None, None, None) == _lib.GF3_EINVAL
    assert lib.gf3_noise_estimate_cs(eng._h, ptr, 65536, ptr, ptr, None) == _lib.GF3_EINVAL
    assert b"65535" in lib.gf3_last_error(eng._h)
    assert lib.gf3_soft_demap_nw_cs(eng._h, ptr, ptr, ptr, 65536, 0, ptr, None) == _lib.GF3_EINVAL
    assert lib.gf3_soft_demap_nw_cs(eng._h, ptr, ptr, ptr, 1, 2, ptr, None) == _lib.GF3_EINVAL
    assert b"gf3_soft_demap_nw_cs" in lib.gf3_last_error(eng._h)
    assert lib.gf3_interleave(eng._h, ptr, ptr, 1, 4, 0, None) == _lib.GF3_EINVAL          # in place
    assert lib.gf3_interleave(eng._h, ptr, None, 1, 2, 0, None) == _lib.GF3_EINVAL
    assert lib.gf3_interleave(eng._h, ptr, None, 65536, 4, 0, None) == _lib.GF3_EINVAL


# ---- end to end through the façade ------------------------------------------------------------------------------
SNR_DB = 15.0
CLICKED = (70, 71, 72)                                     # data symbols of packet 0: far from the pilots and the chirp
CLICK = 8.0                                                # click amplitude, in units of the signal's rms


def clicked(sig, tx, start, scale, seed=5):
    """White noise SNR_DB below the signal's power; the samples of the data symbols CLICKED (prefix included) are
    OVERWRITTEN with white noise of CLICK x scale times the signal's rms."""
    rng = np.random.default_rng(seed)
    rms = np.sqrt(np.mean(sig[2000:-2000] ** 2))
    out = sig + rng.normal(0, rms / 10 ** (SNR_DB / 20), sig.shape)
    S = tx.ofdm_symbol_size + tx.cp_length
    for l in CLICKED:
        a = start + (tx.no_pilots + l) * S
        out[a: a + S] = rng.normal(0, CLICK * scale * rms, S)
    return out


def restated(noisy, start, coded, n_cw, p, shifts, interleaved):
    """The same samples through the oracle's demodulation, the weightings in NumPy and the restated decoder.
    -> (failed codewords per weighting, symbol snr_db [D])"""
    o = orc.demod_frames(noisy, np.array([start]), p)
    eq = o["eq"]
    var_c, var_s = IR.noise_estimate2(eq, p.const_points, p.D)
    llrs = {"noise": NR.soft_demap_nw(eq, var_c, p.const_points, p.const_bits, p.D),
            "noise2d": IR.soft_demap_nw2(eq, var_c, var_s, p.const_points, p.const_bits)}
    cw = coded[: n_cw * 1536].reshape(n_cw, 1536)
    failed = {}
    for name, llr in llrs.items():
        if interleaved:
            llr = IR.deinterleave(llr, p.D, p.C, p.mu)
        bits, _, it = R.decode(shifts, llr[: cw.size].reshape(cw.shape), 50)
        failed[name] = int(np.sum((bits != cw[:, : bits.shape[1]]).any(axis=1) | (it < 0)))
    return failed, IR.symbol_snr_db(var_c, var_s, p.const_points)[0]


def test_facade_interleaver_with_symbol_weights_survives_three_clicked_symbols():
    """Mode A2, "QCLDPC-1/2", 150 000 payload bits (196 codewords in one packet), white noise 15 dB below the signal, and
    data symbols 70-72 of the packet overwritten with white noise of 8 x the signal's rms (x0.8 / x1 / x1.2).

    The levels are restated on this test's own samples before the GPU is looked at: in stream order the three symbols
    hold 8400 adjacent coded bits, five to six codewords that no weighting saves; interleaved with per-carrier weights the
    garbage is spread, unmarked, over every codeword; interleaved with carrier x symbol weights every codeword loses
    ~26 of 1536 bits as near-erasures and decodes.  Restated failed codewords of 196 on these samples, "noise" | "noise2d",
    the same at x0.8 / x1 / x1.2: stream order 7 | 5, interleaved 196 | 0; symbol SNR -18.0 / -20.0 / -21.8 dB on the clicked
    symbols against a median of 12.1 dB."""
    from gf3_audio_modem_amd.OFDM import receiver
    from gf3_audio_modem_amd.ldpc import shift_table
    rng = np.random.default_rng(2026)
    payload = rng.integers(0, 2, size=150_000)
    sh = shift_table("1/2")
    n_cw = -(-len(payload) // 768)
    streams = {}
    for inter in (False, True):
        np.random.seed(17)
        tx = receiver("A2", encoding="QCLDPC-1/2")
        tx.interleave = inter
        coded = np.asarray(tx.encode(payload))
        np.random.seed(17)
        sig = tx.transmit(payload)
        streams[inter] = (coded, np.concatenate([np.zeros(2000), sig, np.zeros(2000)]))
    # encode() with the interleaver == the restated permutation of encode() without it (same seed: same fill)
    assert np.array_equal(streams[True][0], IR.interleave(streams[False][0].reshape(-1, 504000), 180, 1400, 2).reshape(-1))
    p = modeA2_params(np.asarray(tx.known_sequence[: tx.K * tx.mu], dtype=np.uint8))
    start = 2000 + tx.chirp_length
    for scale in (0.8, 1.2, 1.0):                          # (ends on the streams the GPU receives)
        noisy = {}
        for inter in (False, True):
            coded, sig = streams[inter]
            noisy[inter] = clicked(sig, tx, start, scale)
            plain = IR.deinterleave(coded.reshape(-1, 504000), 180, 1400, 2).reshape(-1) if inter else coded
            failed, snr_s = restated(noisy[inter], start, plain.astype(np.uint8), n_cw, p, sh, inter)
            print(f"click x{scale}, interleave={inter}: restated failed codewords of {n_cw} {failed}, "
                  f"symbol snr_db median {np.median(snr_s):.2f}, clicked {np.round(snr_s[list(CLICKED)], 2)}")
            if inter:
                assert failed["noise"] > 0 and failed["noise2d"] == 0
            else:
                assert failed["noise"] > 0 and failed["noise2d"] > 0
            assert sorted(np.argsort(snr_s)[:3].tolist()) == list(CLICKED)

    rx = receiver("A2", encoding="QCLDPC-1/2")
    assert rx.interleave is False and rx.last_symbol_snr_db is None
    rx.llr_weighting = "noise"
    out, _, _ = rx.receive(noisy[False])
    assert not np.array_equal(out[: len(payload)], payload)                # stream order: whole codewords are gone
    assert rx.last_symbol_snr_db is None
    rx.interleave = True
    out, _, _ = rx.receive(noisy[True])
    assert not np.array_equal(out[: len(payload)], payload)                # spread, unmarked: worse
    rx.llr_weighting = "noise2d"
    out, Hs0, _ = rx.receive(noisy[True])
    assert out.dtype == np.int64 and Hs0.shape == (2047,)
    assert np.array_equal(out[: len(payload)], payload)
    snr, snr_l = rx.last_snr_db, rx.last_symbol_snr_db
    assert snr.dtype == snr_l.dtype == np.float64 and snr.shape == (1, 1400) and snr_l.shape == (1, 180)
    assert sorted(np.argsort(snr_l[0])[:3].tolist()) == list(CLICKED)
    np.testing.assert_allclose(snr_l[0], snr_s, atol=1e-6)                 # (engine and oracle agree on eq to ~1e-9)

    # the hard chain on a clean interleaved stream; its guards
    clean = streams[True][1]
    raw, _, _ = receiver("A2", encoding="None").receive(clean)
    assert np.array_equal(raw, streams[True][0])
    dec = rx.decode(rx.PS(raw))
    assert np.array_equal(dec[: len(payload)], payload)
    with pytest.raises(ValueError, match="whole packets"):
        rx.decode(raw[:-1])
    for enc in ("XOR", "None"):
        bad = receiver("A2", encoding=enc)
        bad.interleave = True
        with pytest.raises(ValueError, match="interleave"):
            bad.encode(payload)
        with pytest.raises(ValueError, match="interleave"):
            bad.receive(clean)


def test_defaults_are_unchanged_by_the_new_attributes():
    """interleave = False: "csi" and "noise" return exactly what the direct engine calls return (the form of
    test_default_weighting_is_unchanged_... in tests/test_noise_gpu.py); with interleave = True they return the engine's
    LLRs through the bare inverse permutation."""
    from gf3_audio_modem_amd import QCLDPC
    from gf3_audio_modem_amd.OFDM import receiver
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, size=100_000)
    code = QCLDPC("3/4")
    for inter in (False, True):
        np.random.seed(5)
        tx = receiver("A2", encoding="QCLDPC-3/4")
        tx.interleave = inter
        sig = np.concatenate([np.zeros(2000), tx.transmit(bits), np.zeros(2000)])
        noisy = sig + np.random.default_rng(4).normal(0, np.sqrt(np.mean(sig ** 2) / 10 ** 0.9), sig.shape)
        rx = receiver("A2", encoding="QCLDPC-3/4")
        rx.interleave = inter
        eng = rx._engine(noisy.dtype)
        x = eng._samples(noisy)
        o = eng.demod_frames(x, (eng.sync_stream(x) + 2)[:-1], want=("eq", "Hs", "He"))
        direct = {"csi": eng.soft_demap_csi(o["eq"], o["Hs"], o["He"]),
                  "noise": eng.soft_demap_nw(o["eq"], eng.noise_estimate(o["eq"]))}
        for weighting, llr in direct.items():
            rx.llr_weighting = weighting
            got, _, _ = rx.receive(noisy)
            if inter:
                llr = eng.interleave(llr, inverse=True)
            want = code.decode(llr[: llr.numel() // code.n * code.n], max_iter=rx.ldpc_max_iter).reshape(-1).cpu().numpy()
            assert np.array_equal(got, want.astype(np.int64)), (inter, weighting)
    rx.llr_weighting = "noise2d"
    rx.host_chunk_samples = 1 << 20
    with pytest.raises(NotImplementedError, match="piece-wise host path"):
        rx.receive(noisy)
    rx.llr_weighting = "2d"
    with pytest.raises(ValueError, match="llr_weighting"):
        rx.receive(noisy)
