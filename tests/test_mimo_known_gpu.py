"""The known-bit joint detector on the GPU (gf3_mimo_detect_known, Engine.mimo_detect_known) against Engine.mimo_detect's
bytes where nothing is known and against the NumPy restatement (tests/mimo_known_ref.py) where something is; edge inputs and
argument checks; and transmit_mimo -> the scenario's room -> receive_mimo under `mimo_cancellation` end to end, at the level
tests/test_mimo_known_cpu.py settles.  The guard-band rows of the entry are in tests/test_bounds_mimo_known_gpu.py.

Base shape: N = 1024, P = 2, D = 5, data bins 5 .. 399 (C = 395: two 256-carrier tiles, the second partial), F = 2."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import mimo_known_ref as KR
from tests import mimo_ref as MR
from tests import tables as T
from tests.test_mimo_gpu import LEAD, TAIL, detect_inputs, engine_of, facade, oracle_params, quiet, same_bytes, small_params
from tests.test_mimo_known_cpu import LEVEL_DB

pytestmark = pytest.mark.gpu
F2, D5 = 2, 5
RUN = 1536                                                  # a codeword of the default block length
PATTERNS = ("stream0", "stream1", "runs", "single")
E2E_SEEDS = (14, 114)                                       # noise seeds of the end-to-end case (microphone 0, 1)


def planes(eng, bits, known):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)).to(eng.device)
    return dev(bits), dev(known)


def masks(pattern, shape, seed):
    """-> (bits, known) uint8 of `shape` = (F, 2, D, C, 2): seeded bits, and what is known of them under `pattern`"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, size=shape).astype(np.uint8)
    known = np.zeros(shape, dtype=np.uint8)
    if pattern == "stream0":
        known[:, 0] = 1
    elif pattern == "stream1":
        known[:, 1] = 1
    elif pattern == "runs":                                 # a random half of the codeword-sized runs; the tail past them unknown
        n = bits.size // RUN
        flat = known.reshape(-1)
        for i in rng.permutation(n)[: n // 2]:
            flat[i * RUN: (i + 1) * RUN] = 1
    elif pattern == "single":
        known[...] = rng.random(size=shape) < 0.3
    else:
        assert pattern == "none"
    return bits, known


def held(got, ref, known, bits, what=""):
    """The detector tests' own tolerance on the unknown bits, exactly -+GF3_LLR_KNOWN on the known ones"""
    free = known == 0
    atol = 1e-9 * np.abs(ref[free]).max() if free.any() else 0.0
    print(f"{what}: {int(free.sum())} unknown bits, worst deviation {np.abs(got[free] - ref[free]).max() if free.any() else 0:.2e} "
          f"at max |ref| {np.abs(ref[free]).max() if free.any() else 0:.2e}")
    np.testing.assert_allclose(got[free], ref[free], rtol=1e-6, atol=atol)
    want = np.where(bits[~free] != 0, -KR.LLR_KNOWN, KR.LLR_KNOWN)
    assert np.array_equal(got[~free].view(np.uint32), want.view(np.uint32))


@functools.lru_cache(maxsize=None)
def base(table="qpsk_ref"):
    p = small_params(P=2, D=D5, table=T.TABLES[table])
    return p, engine_of(p), detect_inputs(p, F2, 4, 77)


def weights_for(p, F, B, seed=5):
    return np.exp(np.random.default_rng(seed).normal(size=(B, F, p.C)))


# ---- nothing known: the bytes of the plain detector ------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_nothing_known_gives_the_bytes_of_mimo_detect(B, weighted):
    p, eng, (Ys, Hs, slopes) = base()
    Ys, Hs, slopes = Ys[:B], Hs[:B], slopes[:B]
    w = weights_for(p, F2, B) if weighted else None
    plain = eng.mimo_detect(Ys, Hs, slopes, weights=w)
    bits, known = planes(eng, *masks("none", (F2, 2, p.D, p.C, 2), B))
    got = eng.mimo_detect_known(Ys, Hs, slopes, bits, known, weights=w)
    assert got.dtype == torch.float32 and got.shape == plain.shape == (F2, 2, p.D, p.C, 2)
    assert same_bytes(got, plain)
    assert np.abs(plain.cpu().numpy()).max() > 0


# ---- something known: the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["qpsk_ref", "qpsk_rot"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("B", [2, 4])
def test_known_bits_against_the_restatement(B, pattern, table):
    p, eng, (Ys, Hs, slopes) = base(table)
    Ys, Hs, slopes = Ys[:B], Hs[:B], slopes[:B]
    bits, known = masks(pattern, (F2, 2, p.D, p.C, 2), 10 * B + PATTERNS.index(pattern))
    got = eng.mimo_detect_known(Ys, Hs, slopes, *planes(eng, bits, known))
    ref = KR.detect_known(Ys, Hs, slopes, p, bits, known)
    held(got.cpu().numpy(), ref, known, bits, f"B {B}, {pattern}, {table}")
    assert same_bytes(got, eng.mimo_detect_known(Ys, Hs, slopes, *planes(eng, bits, known)))       # two calls, identical bytes
    if pattern == "single":                                     # the weighted metric under the same masks
        w = weights_for(p, F2, B)
        got = eng.mimo_detect_known(Ys, Hs, slopes, *planes(eng, bits, known), weights=w)
        held(got.cpu().numpy(), KR.detect_known(Ys, Hs, slopes, p, bits, known, w), known, bits, f"B {B}, {pattern}, {table}, weighted")


def test_runs_of_symbols_per_workgroup():
    """32 packet pairs of 100 symbols on the carriers 5 .. 261 (two carrier tiles, the second holding one carrier): a workgroup
    takes a run of 4 consecutive symbols on 256 compute units, phasors and mask reads advancing with it; three pairs are held
    to the restatement, all to the plain detector's bytes where nothing is known."""
    p = small_params(P=2, D=100, carriers=np.arange(5, 262))
    eng = engine_of(p)
    F = 32
    Ys, Hs, slopes = detect_inputs(p, F, 2, 61)
    bits, known = masks("single", (F, 2, p.D, p.C, 2), 3)
    known[5] = 0
    got = eng.mimo_detect_known(Ys, Hs, slopes, *planes(eng, bits, known)).cpu().numpy()
    assert np.array_equal(got[5].view(np.uint32), eng.mimo_detect(Ys, Hs, slopes).cpu().numpy()[5].view(np.uint32))
    packets = np.array([0, 17, 31])
    rows = (packets[:, None] * p.D + np.arange(p.D)).reshape(-1)
    ref = KR.detect_known([y[rows] for y in Ys], [h[packets] for h in Hs], [s[packets] for s in slopes], p, bits[packets], known[packets])
    held(got[packets], ref, known[packets], bits[packets], "D 100, 257 carriers")


@pytest.mark.parametrize("N", [2048, 4096, 8192])
def test_known_bits_at_the_other_transform_sizes(N):
    p = small_params(P=2, D=2, N=N)
    eng = engine_of(p)
    Ys, Hs, slopes = detect_inputs(p, 2, 2, N)
    bits, known = masks("single", (2, 2, p.D, p.C, 2), N)
    got = eng.mimo_detect_known(Ys, Hs, slopes, *planes(eng, bits, known))
    held(got.cpu().numpy(), KR.detect_known(Ys, Hs, slopes, p, bits, known), known, bits, f"N {N}")


def test_edge_inputs():
    """A NaN in Y and an Inf in H at known and at unknown cells, a zero and a non-finite weight, a non-finite slope, and mask
    bytes of 255 / bit bytes of 2, which read as non-zero."""
    p, eng, (Ys, Hs, slopes) = base()
    Ys, Hs, slopes = [y.copy() for y in Ys[:2]], [h.copy() for h in Hs[:2]], [s.copy() for s in slopes[:2]]
    shape = (F2, 2, p.D, p.C, 2)
    bits, known = masks("single", shape, 21)
    bins = p.data_carriers
    cell = lambda f, l: f * p.D + l
    known[0, :, 3, 17], known[0, :, 3, 18] = 1, 0           # a NaN in one branch's y at a known cell and at an unknown one
    Ys[0][cell(0, 3), bins[17]] = Ys[0][cell(0, 3), bins[18]] = complex(np.nan, 0.0)
    known[1, :, :, 40], known[1, :, :, 41] = 1, 0           # an Inf in one estimate: that carrier of that pair, every symbol
    Hs[1][1, 0, 1, bins[40] - 1] = Hs[1][1, 1, 0, bins[41] - 1] = complex(np.inf, 0.0)
    known[1, :, 4, 300], known[1, :, 4, 301] = 1, 0         # every branch: nothing is left
    for y in Ys:
        y[cell(1, 4), bins[300]] = y[cell(1, 4), bins[301]] = complex(np.nan, np.nan)
    raw_b, raw_k = bits * 2, known * 255                    # (non-zero bytes other than 1)
    got = eng.mimo_detect_known(Ys, Hs, slopes, *planes(eng, raw_b, raw_k)).cpu().numpy()
    assert np.isfinite(got).all()
    held(got, KR.detect_known(Ys, Hs, slopes, p, bits, known), known, bits, "planted non-finites")
    assert same_bytes(torch.from_numpy(got), eng.mimo_detect_known(Ys, Hs, slopes, *planes(eng, bits, known)))
    dead = got[1, :, 4, 301]
    assert not dead.any() and not np.signbit(dead).any()
    assert np.array_equal(np.abs(got[1, :, 4, 300]), np.full((2, 2), KR.LLR_KNOWN))
    # weights: a zero takes the branch out at the carrier, a non-finite one too; both branches out: +0 / -+constant
    w = weights_for(p, F2, 2)
    w[0, 0, 7], w[1, 0, 9], w[:, 1, 11], w[0, 1, 12], w[1, 1, 12] = 0.0, np.nan, 0.0, np.inf, 0.0
    got = eng.mimo_detect_known(Ys, Hs, slopes, *planes(eng, bits, known), weights=w).cpu().numpy()
    held(got, KR.detect_known(Ys, Hs, slopes, p, bits, known, w), known, bits, "planted weights")
    for c in (11, 12):
        free = known[1, :, :, c] == 0
        assert not got[1, :, :, c][free].any() and not np.signbit(got[1, :, :, c][free]).any()
    # a non-finite slope in every branch of pair 0: +0 on its unknown bits, -+constant on its known ones
    for s in slopes:
        s[0] = np.nan
    got = eng.mimo_detect_known(Ys, Hs, slopes, *planes(eng, bits, known)).cpu().numpy()
    free = known[0] == 0
    assert not got[0][free].any() and not np.signbit(got[0][free]).any()
    assert np.array_equal(got[0][~free], np.where(bits[0][~free] != 0, -KR.LLR_KNOWN, KR.LLR_KNOWN))
    held(got[1:], KR.detect_known([y[p.D:] for y in Ys], [h[1:] for h in Hs], [s[1:] for s in slopes], p, bits[1:], known[1:]),
         known[1:], bits[1:], "pair 1 beside a dead pair")


def test_argument_checks():
    from gf3_audio_modem_amd import _lib
    p, eng, (Ys, Hs, slopes) = base()
    Ys, Hs, slopes = Ys[:2], Hs[:2], slopes[:2]
    n = F2 * 2 * p.D * p.C * 2
    bits, known = planes(eng, *masks("single", (F2, 2, p.D, p.C, 2), 1))
    good = dict(Ys=Ys, Hs=Hs, slopes=slopes, bits=bits, known=known)
    bad = [dict(Ys=[]), dict(Hs=Hs[:1]), dict(Ys=[y[:-1] for y in Ys]), dict(bits=None), dict(known=None), dict(bits=bits[:-1]),
           dict(known=torch.cat([known, known])), dict(bits=bits.to(torch.int32)), dict(known=known.cpu()), dict(bits=bits.cpu().numpy()),
           dict(known=torch.cat([known, known])[::2]), dict(out=torch.empty(n - 1, dtype=torch.float32, device="cuda")),
           dict(weights=np.ones((2, F2, p.C - 1)))]
    for kw in bad:
        with pytest.raises(ValueError, match="mimo_detect_known"):
            eng.mimo_detect_known(**{**good, **kw})
    # F = 0 leaves `out` untouched
    out = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    e = eng.mimo_detect_known([np.zeros((0, 513), complex)] * 2, [np.zeros((0, 2, 2, 511), complex)] * 2, [np.zeros(0)] * 2, empty, empty)
    assert e.shape == (0, 2, p.D, p.C, 2)
    o = eng.mimo_detect_known(**good, out=out)
    assert o.data_ptr() == out.data_ptr() and same_bytes(o, eng.mimo_detect_known(**good))
    # a 16-QAM context: the façade and the library both refuse
    e16 = engine_of(small_params(P=2, D=D5, table=orc.square_qam_table(4)))
    with pytest.raises(ValueError, match="mimo_detect_known.*mu = 2"):
        e16.mimo_detect_known(**good)
    # the raw ABI
    lib = eng.lib
    dY, dH = [eng._dev(y) for y in Ys], [eng._dev(h) for h in Hs]
    dS = [eng._dev(s, torch.float64) for s in slopes]
    dW = eng._dev(weights_for(p, F2, 2), torch.float64)
    tab = lambda xs: (C.c_void_p * len(xs))(*[None if x is None else x.data_ptr() for x in xs])
    Yt, Ht, St, q, bp, kp, wp = tab(dY), tab(dH), tab(dS), _lib.ptr(out), _lib.ptr(bits), _lib.ptr(known), _lib.ptr(dW)
    call = lambda *a: lib.gf3_mimo_detect_known(*a, None)
    out.fill_(7.0)
    assert call(eng._h, 2, Yt, Ht, St, None, bp, kp, 0, q) == 0 and call(eng._h, 9, None, None, None, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                   # F == 0: a no-op
    assert call(eng._h, 2, Yt, Ht, St, wp, bp, kp, F2, q) == 0 and call(eng._h, 2, Yt, Ht, St, None, bp, kp, F2, q) == 0
    F = F2
    cases = {"no context": (None, 2, Yt, Ht, St, None, bp, kp, F, q), "B = 0": (eng._h, 0, Yt, Ht, St, None, bp, kp, F, q),
             "B = 5": (eng._h, 5, Yt, Ht, St, None, bp, kp, F, q), "no spectra": (eng._h, 2, None, Ht, St, None, bp, kp, F, q),
             "no estimates": (eng._h, 2, Yt, None, St, None, bp, kp, F, q), "no slopes": (eng._h, 2, Yt, Ht, None, None, bp, kp, F, q),
             "null spectrum": (eng._h, 2, tab([dY[0], None]), Ht, St, None, bp, kp, F, q),
             "null estimate": (eng._h, 2, Yt, tab([None, dH[1]]), St, wp, bp, kp, F, q),
             "null slope": (eng._h, 2, Yt, Ht, tab([dS[0], None]), None, bp, kp, F, q),
             "no bits": (eng._h, 2, Yt, Ht, St, None, None, kp, F, q), "no mask": (eng._h, 2, Yt, Ht, St, wp, bp, None, F, q),
             "no output": (eng._h, 2, Yt, Ht, St, None, bp, kp, F, None), "F < 0": (eng._h, 2, Yt, Ht, St, None, bp, kp, -1, q),
             "too many packets": (eng._h, 2, Yt, Ht, St, None, bp, kp, 65536, q), "16-QAM": (e16._h, 2, Yt, Ht, St, None, bp, kp, F, q)}
    for text, args in cases.items():
        assert call(*args) == _lib.GF3_EINVAL, text
        assert b"gf3_mimo_detect_known" in lib.gf3_last_error(None), text
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------------------------------
CODEWORDS = 9


@functools.lru_cache(maxsize=None)
def coded_recordings():
    """One packet pair of 9 rate-1/2 codewords with their CRC through transmit_mimo and the scenario's room, noiseless
    -> (payload, stereo signal, [mic 0, mic 1])"""
    rx = facade("QCLDPC-1/2", codeword_crc=True)
    payload = np.random.default_rng(3).integers(0, 2, size=CODEWORDS * (768 - 32))
    np.random.seed(5)
    tx2 = quiet(rx.transmit_mimo, payload)
    assert rx.no_packets == 2
    tx2 = np.concatenate([np.zeros((2, LEAD)), tx2, np.zeros((2, TAIL))], axis=1)
    return payload, tx2, MR.through(tx2)


@functools.lru_cache(maxsize=None)
def noisy():
    payload, tx2, rec = coded_recordings()
    return KR.add_noise(rec, tx2, LEVEL_DB, E2E_SEEDS)


@functools.lru_cache(maxsize=None)
def restated():
    """The restated chain on the same samples -> (untrusted after the first decode, at the end, passes run)"""
    from gf3_audio_modem_amd.ldpc import shift_table
    rx = facade("QCLDPC-1/2", codeword_crc=True)
    res, _ = KR.receive(noisy(), oracle_params(rx), shift_table("1/2"), CODEWORDS, 2, crc=True)
    return res["first"], res["left"], res["passes"]


def received(**attrs):
    rx = facade("QCLDPC-1/2", codeword_crc=True, **attrs)
    bits, _, _ = quiet(rx.receive_mimo, noisy())
    rep = rx.last_decode_report
    return bits, rep, rep["inner_failed"] + rep["crc_failed"]


def test_receive_mimo_cancels_at_the_settled_level():
    """Mode A3, no_pilots 4, packet_length 4, "QCLDPC-1/2" with the codeword CRC, LEVEL_DB, noise seeds E2E_SEEDS.  The
    report's untrusted codewords (given up, or converged on a wrong CRC) are the restated chain's, before and after.
    Measured on an MI355X: 4 untrusted of 9 after the first decode, 3 after 2 passes, GPU and restatement alike (and alike
    at every seed s = 0 .. 29 of (s, s + 100): DESIGN §12)."""
    payload, _, _ = coded_recordings()
    first, left, passes = restated()
    print(f"restated: untrusted {first} -> {left} of {CODEWORDS} in {passes} passes")
    assert first - left >= 1
    _, rep0, untrusted0 = received(mimo_cancellation=0)
    assert rep0["codewords"] == CODEWORDS and "cancel_passes" not in rep0 and "cancel_recovered" not in rep0
    bits, rep2, untrusted2 = received(mimo_cancellation=2)
    print(f"GPU: untrusted {untrusted0} -> {untrusted2}, report {rep2}")
    assert untrusted0 == first
    assert untrusted2 == left and rep2["cancel_recovered"] == first - left and rep2["cancel_passes"] == passes
    k = 768 - 32
    good = [i for i in range(CODEWORDS) if i not in set(rep2["failed_codewords"]) | set(rep2["crc_failed_codewords"])]
    for i in good:
        assert np.array_equal(bits[i * k: (i + 1) * k], payload[i * k: (i + 1) * k]), i


def test_receive_mimo_cancels_under_noise_weighting():
    """The same samples under joint_weighting = "noise" (P = 4): the passes run under the call's weights and recover at
    least what the unweighted call does.  Measured: 5 -> 3 untrusted (2 recovered) against 4 -> 3 (1 recovered)."""
    _, rep_csi, _ = received(mimo_cancellation=2)
    _, rep0, untrusted0 = received(mimo_cancellation=0, joint_weighting="noise")
    _, rep2, untrusted2 = received(mimo_cancellation=2, joint_weighting="noise")
    print(f"joint_weighting 'noise': untrusted {untrusted0} -> {untrusted2}, report {rep2}; 'csi' recovered {rep_csi['cancel_recovered']}")
    assert rep2["cancel_recovered"] == untrusted0 - untrusted2
    assert rep2["cancel_recovered"] >= rep_csi["cancel_recovered"]


def test_noiseless_runs_no_pass():
    payload, _, rec = coded_recordings()
    out = []
    for n in (0, 2):
        rx = facade("QCLDPC-1/2", codeword_crc=True, mimo_cancellation=n)
        bits, _, _ = quiet(rx.receive_mimo, rec)
        out.append((bits, rx.last_decode_report))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[1][0][: len(payload)], payload)
    assert out[1][1]["cancel_passes"] == 0 and out[1][1]["cancel_recovered"] == 0 and out[1][1]["inner_failed"] == 0
    assert "cancel_passes" not in out[0][1]
