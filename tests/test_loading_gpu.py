"""Adaptive bit loading on the GPU: gf3_noise_estimate_loaded / gf3_soft_demap_loaded against the NumPy restatement
(tests/loading_ref.py) and, on uniform loadings, bit for bit against the uniform kernels; their edge inputs and
refusals; and the loop probe -> allocation -> loaded round trip through the façade on a channel whose SNR falls over the band."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import loading_ref as LR
from tests import noise_ref as NR
from tests import tables as T
from tests.test_loading_cpu import patterns
from tests.util import engine_for

pytestmark = pytest.mark.gpu
N, K, P = 1024, 511, 2


def contiguous(C):
    return np.arange(7, 7 + C)


# name -> (order, bins, D, F)
CASES = {
    "mixed": (patterns()["mixed"], contiguous(130), 3, 2),                  # C = 130: no multiple of 64
    "zeros": (patterns()["zeros"], contiguous(130), 3, 2),                  # first and last carrier off; carriers 58 .. 127 off: the wave 64 .. 127 holds zeros only
    "single": (patterns()["single"], np.array([300]), 5, 2),                # C = 1
    "long": (patterns()["mixed"], contiguous(130), 37, 1),                  # many one-symbol chunks; waves with 4 and 5 symbols
    "short": (patterns()["mixed"], contiguous(130), 2, 3),                  # fewer symbols than waves
    "shuffled": (patterns()["cycle"], T.shuffled(K), 3, 2),                 # a scattered map: the CSI weight's bin look-up
}


@functools.lru_cache(maxsize=None)
def setup(C_key, D, m=0):
    """(p, engine) on the carrier map of CASES[C_key]; the context's table is the reference's QPSK (m = 0) or
    square_qam_table(m)."""
    bins = CASES[C_key][1]
    pts, bits = orc.qpsk_table() if m == 0 else orc.square_qam_table(m)
    mu = bits.shape[1]
    known = np.random.default_rng(5).integers(0, 2, K * mu).astype(np.uint8)
    p = orc.RxParams(N=N, CP=0, P=P, D=D, carriers=np.asarray(bins), const_points=pts, const_bits=bits.astype(np.int64),
                     known_bits=known, fit_lo=10, fit_hi=100)
    return p, engine_for(p)


def known_of(eng):
    return eng.cfg.known_symbols()[np.asarray(eng.cfg.data_bins) - 1]


@functools.lru_cache(maxsize=None)
def case(name):
    """One case's inputs and restated outputs, computed once: noisy symbols (a noise level per carrier, so that the
    variances differ), random Hs / He, the restated variances and the LLRs of the three weights."""
    order, bins, D, F = CASES[name]
    p, eng = setup(name, D)
    rng = np.random.default_rng(len(name) + D)
    C = len(order)
    Bs, _ = LR.layout(order)
    known = known_of(eng)
    bits = rng.integers(0, 2, F * D * Bs)
    clean = LR.map_loaded(bits, order, known)
    sig = 0.01 + 0.05 * rng.random(C)
    eq = clean + (rng.normal(size=clean.shape) + 1j * rng.normal(size=clean.shape)) * sig
    Hs = rng.normal(size=(F, K)) + 1j * rng.normal(size=(F, K))
    He = Hs * (1.0 + 0.2 * rng.normal(size=(F, K))) + 0.1j * rng.normal(size=(F, K))
    var = LR.noise_estimate(eq, order, known, D)
    ref = {"unit": LR.soft_demap(eq, order, D), "var": LR.soft_demap_nw(eq, var, order, D),
           "csi": LR.soft_demap_csi(eq, Hs, He, bins, order, P, D)}
    for a in (eq, clean, Hs, He, var, bits, *ref.values()):
        a.setflags(write=False)
    return dict(order=order, bins=bins, D=D, F=F, C=C, Bs=Bs, eng=eng, known=known, bits=bits, clean=clean, eq=eq, Hs=Hs, He=He,
                var=var, ref=ref)


def three(eng, ld, eq, Hs, He, var):
    return {"unit": eng.soft_demap_loaded(eq, ld), "var": eng.soft_demap_loaded(eq, ld, var=var),
            "csi": eng.soft_demap_loaded(eq, ld, Hs=Hs, He=He)}


@pytest.mark.parametrize("name", list(CASES))
def test_loaded_pair_matches_restatement(name):
    c = case(name)
    eng = c["eng"]
    ld = eng.loading(c["order"])
    assert ld.bits == c["Bs"] and eng.loading(c["order"].astype(np.int64)) is ld           # cached by the table's bytes
    var = eng.noise_estimate_loaded(c["eq"], ld)
    assert var.dtype == torch.float64 and tuple(var.shape) == (c["F"], c["C"]) and c["var"].min() > 0
    np.testing.assert_allclose(var.cpu().numpy(), c["var"], rtol=1e-12, atol=0)
    again = eng.noise_estimate_loaded(c["eq"], c["order"])
    assert np.array_equal(var.cpu().numpy().view(np.int64), again.cpu().numpy().view(np.int64))
    got = three(eng, ld, c["eq"], c["Hs"], c["He"], var)
    for kind, llr in got.items():
        ref = c["ref"][kind]
        llr = llr.cpu().numpy()
        assert llr.dtype == np.float32 and llr.shape == ref.shape == (c["F"] * c["D"] * c["Bs"],)
        np.testing.assert_allclose(llr, ref, rtol=1e-6, atol=1e-9 * np.abs(ref).max(), err_msg=kind)
    twice = three(eng, ld, c["eq"], c["Hs"], c["He"], var)
    for kind in got:
        assert np.array_equal(got[kind].cpu().numpy().view(np.int32), twice[kind].cpu().numpy().view(np.int32)), kind
    # a noiseless copy: the signs are the mapped bits under every weight, and no residual is left
    clean = three(eng, ld, c["clean"], c["Hs"], c["He"], c["var"])
    for kind, llr in clean.items():
        assert np.array_equal(LR.hard_bits(llr.cpu().numpy()), c["bits"]), kind
    assert eng.noise_estimate_loaded(c["clean"], ld).abs().max().item() < 1e-30


@pytest.mark.parametrize("m", [2, 4, 6])
def test_uniform_loading_is_the_uniform_kernels_bit_for_bit(m):
    """A context of square_qam_table(m) and an all-m loading: the estimate and the noise-weighted LLRs are the parent
    kernels' bits; the CSI-weighted LLRs round once where the staged pair (soft demapper, then the weight) rounds twice:
    within 1.5 x 2^-23 relative, the relation gf3_demod_frames_llr's header states."""
    D, F = 11, 2
    p, eng = setup("mixed", D, m)
    C = p.C
    rng = np.random.default_rng(m)
    pts = p.const_points
    eq = pts[rng.integers(0, len(pts), (F * D, C))] + (rng.normal(size=(F * D, C)) + 1j * rng.normal(size=(F * D, C))) * (0.02 + 0.1 * rng.random(C))
    Hs = rng.normal(size=(F, K)) + 1j * rng.normal(size=(F, K))
    He = rng.normal(size=(F, K)) + 1j * rng.normal(size=(F, K))
    ld = eng.loading(np.full(C, m, dtype=np.uint8))
    v0, v1 = eng.noise_estimate(eq), eng.noise_estimate_loaded(eq, ld)
    assert np.array_equal(v0.cpu().numpy().view(np.int64), v1.cpu().numpy().view(np.int64))
    l0, l1 = eng.soft_demap_nw(eq, v0), eng.soft_demap_loaded(eq, ld, var=v1)
    assert l0.numel() == l1.numel() == F * D * C * m
    assert np.array_equal(l0.cpu().numpy().view(np.int32), l1.cpu().numpy().view(np.int32))
    u0, u1 = eng.soft_demap(eq, 1.0).reshape(-1), eng.soft_demap_loaded(eq, ld)
    assert np.array_equal(u0.cpu().numpy().view(np.int32), u1.cpu().numpy().view(np.int32))
    c0 = eng.soft_demap_csi(eq, Hs, He).cpu().numpy().astype(np.float64)
    c1 = eng.soft_demap_loaded(eq, ld, Hs=Hs, He=He).cpu().numpy().astype(np.float64)
    assert (np.abs(c1 - c0) <= 1.5 * 2.0 ** -23 * np.abs(c0)).all()


def test_nonfinite_symbols_and_flat_packets():
    c = case("mixed")
    eng, order, D, F, C, Bs = c["eng"], c["order"], c["D"], c["F"], c["C"], c["Bs"]
    ld = eng.loading(order)
    _, off = LR.layout(order)
    eq = c["eq"].copy()
    a, b, z = 10, 63, 64                                   # orders 2, 6 and 0
    assert (order[a], order[b], order[z]) == (2, 6, 0)
    eq[D + 1, a] = complex(np.nan, 0.0)                    # packet 1
    eq[D, b] = complex(0.5, -np.inf)
    var = eng.noise_estimate_loaded(eq, ld).cpu().numpy()
    ref_v = LR.noise_estimate(eq, order, c["known"], D)
    fin = np.isfinite(ref_v)
    assert np.array_equal(np.isfinite(var), fin) and not fin[1, [a, b]].any() and fin.sum() == fin.size - 2
    np.testing.assert_allclose(var[fin], ref_v[fin], rtol=1e-12, atol=0)
    llr = eng.soft_demap_loaded(eq, ld, var=var).cpu().numpy()
    ref = LR.soft_demap_nw(eq, var, order, D)
    assert np.isfinite(llr).all()
    np.testing.assert_allclose(llr, ref, rtol=1e-6, atol=1e-9 * np.abs(ref).max())
    rows = llr.reshape(F, D, Bs)
    for cc in (a, b):
        erased = rows[1][:, off[cc]: off[cc + 1]]
        assert not erased.any() and not np.signbit(erased).any()                  # +0.0f on every symbol
    # packet 0 is untouched by packet 1's symbols
    before = eng.soft_demap_loaded(c["eq"], ld, var=eng.noise_estimate_loaded(c["eq"], ld)).cpu().numpy()
    assert np.array_equal(rows[0].view(np.int32), before.reshape(F, D, Bs)[0].view(np.int32))
    # a noiseless packet: vbar = 0 and the weights are 1
    flat = eng.soft_demap_loaded(c["clean"], ld, var=np.zeros((F, C))).cpu().numpy()
    np.testing.assert_allclose(flat, LR.soft_demap(c["clean"], order, D), rtol=1e-6)
    # a NaN on a carrier of order 0: its variance is not finite, and no LLR of the CSI or unit weights changes (nothing is
    # written for it).  Under the noise weights the rule of gf3_soft_demap_nw is taken literally: vbar, the mean over all C
    # carriers, is then not finite and the packet's weights are 1 -- what the restatement says too.
    eqz = c["eq"].copy()
    eqz[1, z] = complex(np.nan, np.nan)
    vz = eng.noise_estimate_loaded(eqz, ld).cpu().numpy()
    assert not np.isfinite(vz[0, z]) and np.isfinite(np.delete(vz, z, axis=1)).all()
    for kind, kw in (("unit", {}), ("csi", dict(Hs=c["Hs"], He=c["He"]))):
        before = eng.soft_demap_loaded(c["eq"], ld, **kw).cpu().numpy()
        after = eng.soft_demap_loaded(eqz, ld, **kw).cpu().numpy()
        assert np.array_equal(before.view(np.int32), after.view(np.int32)), kind
    nz = eng.soft_demap_loaded(eqz, ld, var=vz).cpu().numpy()
    np.testing.assert_allclose(nz, LR.soft_demap_nw(eqz, vz, order, D), rtol=1e-6, atol=1e-9 * np.abs(ref).max())
    np.testing.assert_allclose(nz.reshape(F, D, Bs)[0], c["ref"]["unit"].reshape(F, D, Bs)[0], rtol=1e-6, atol=1e-9 * np.abs(ref).max())


def test_bounds_out_and_empty_calls():
    c = case("long")
    eng, order, D, F, C, Bs = c["eng"], c["order"], c["D"], c["F"], c["C"], c["Bs"]
    ld = eng.loading(order)
    n = F * D * Bs
    for kw in ({}, dict(var=c["var"]), dict(Hs=c["Hs"], He=c["He"])):
        big = torch.full((n + 1024,), -77.25, dtype=torch.float32, device="cuda")
        out = big[:n]
        assert eng.soft_demap_loaded(c["eq"], ld, out=out, **kw) is out
        assert (big[n:] == -77.25).all().item() and (out != -77.25).all().item()            # every entry written, nothing beyond
    with pytest.raises(ValueError, match="out must be"):
        eng.soft_demap_loaded(c["eq"], ld, out=torch.empty(n + 1, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="eq"):
        eng.soft_demap_loaded(c["eq"][:-1], ld)
    with pytest.raises(ValueError, match="var"):
        eng.soft_demap_loaded(c["eq"], ld, var=c["var"][:, :-1])
    with pytest.raises(ValueError, match="Hs"):
        eng.soft_demap_loaded(c["eq"], ld, Hs=c["Hs"][:, :-1], He=c["He"])
    empty = torch.empty((0, C), dtype=torch.complex128)
    assert tuple(eng.noise_estimate_loaded(empty, ld).shape) == (0, C)
    assert eng.soft_demap_loaded(empty, ld).numel() == 0
    assert eng.soft_demap_loaded(empty, ld, var=torch.empty((0, C), dtype=torch.float64)).numel() == 0


def test_engine_keeps_a_bounded_number_of_loadings():
    """A receiver that allocates anew after every probe: the engine keeps the LOADING_CACHE tables used last; a Loading
    that left the cache is refused, its table is simply made again."""
    c = case("mixed")
    eng, order = c["eng"], c["order"]
    first = eng.loading(order)
    want = eng.soft_demap_loaded(c["eq"], first).cpu().numpy()
    for k in range(eng.LOADING_CACHE - 1):
        other = order.copy()
        other[k] = 6
        eng.loading(other)
        assert eng.loading(order) is first                 # used last: it stays
    assert len(eng._loadings) == eng.LOADING_CACHE
    for k in range(eng.LOADING_CACHE):
        other = order.copy()
        other[k] = 4
        eng.loading(other)
    assert len(eng._loadings) == eng.LOADING_CACHE and first.handle is None
    with pytest.raises(ValueError, match="cache"):
        eng.soft_demap_loaded(c["eq"], first)
    again = eng.soft_demap_loaded(c["eq"], order).cpu().numpy()
    assert eng.loading(order) is not first and np.array_equal(again.view(np.int32), want.view(np.int32))


def test_abi_refusals_name_the_call():
    from gf3_audio_modem_amd import _lib
    c = case("mixed")
    eng, order, D, F, C, Bs = c["eng"], c["order"], c["D"], c["F"], c["C"], c["Bs"]
    lib, h = _lib.load(), eng._h
    ld = eng.loading(order).handle
    eq, Hs, He = eng._dev(c["eq"]), eng._dev(c["Hs"]), eng._dev(c["He"])
    var = eng._dev(c["var"], torch.float64)
    llr = torch.full((F * D * Bs,), 3.5, dtype=torch.float32, device="cuda")
    pt = _lib.ptr

    def refused(rc, name):
        assert rc == _lib.GF3_EINVAL and name in lib.gf3_last_error(h)
    est, dem = lib.gf3_noise_estimate_loaded, lib.gf3_soft_demap_loaded
    refused(est(None, ld, pt(eq), F, pt(var), None), b"gf3_noise_estimate_loaded")
    refused(est(h, None, pt(eq), F, pt(var), None), b"gf3_noise_estimate_loaded")
    refused(est(h, ld, None, F, pt(var), None), b"gf3_noise_estimate_loaded")
    refused(est(h, ld, pt(eq), F, None, None), b"gf3_noise_estimate_loaded")
    refused(est(h, ld, pt(eq), -1, pt(var), None), b"gf3_noise_estimate_loaded")
    refused(est(h, ld, pt(eq), 65536, pt(var), None), b"gf3_noise_estimate_loaded")
    refused(dem(None, ld, pt(eq), None, None, None, F, pt(llr), None), b"gf3_soft_demap_loaded")
    refused(dem(h, None, pt(eq), None, None, None, F, pt(llr), None), b"gf3_soft_demap_loaded")
    refused(dem(h, ld, None, None, None, None, F, pt(llr), None), b"gf3_soft_demap_loaded")
    refused(dem(h, ld, pt(eq), None, None, None, F, None, None), b"gf3_soft_demap_loaded")
    refused(dem(h, ld, pt(eq), None, None, None, -1, pt(llr), None), b"gf3_soft_demap_loaded")
    refused(dem(h, ld, pt(eq), None, None, None, 65536, pt(llr), None), b"gf3_soft_demap_loaded")
    refused(dem(h, ld, pt(eq), pt(Hs), pt(He), pt(var), F, pt(llr), None), b"gf3_soft_demap_loaded")
    refused(dem(h, ld, pt(eq), pt(Hs), None, None, F, pt(llr), None), b"gf3_soft_demap_loaded")
    refused(dem(h, ld, pt(eq), None, pt(He), None, F, pt(llr), None), b"gf3_soft_demap_loaded")
    torch.cuda.synchronize()
    assert (llr == 3.5).all().item()                       # a refused call writes nothing
    # a loading of another context
    _, other = setup("mixed", 37)
    refused(dem(other._h, ld, pt(eq), None, None, None, F, pt(llr), None), b"gf3_soft_demap_loaded")
    # create
    out = ctypes.c_void_p()
    good = np.ascontiguousarray(order)
    as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for bad in (np.full(C, 3, np.uint8), np.full(C, 8, np.uint8), np.zeros(C, np.uint8), np.r_[good[:-1], np.uint8(1)].astype(np.uint8)):
        refused(lib.gf3_loading_create(h, as_p(bad), C, ctypes.byref(out)), b"gf3_loading_create")
        assert not out.value
    refused(lib.gf3_loading_create(h, as_p(good), C - 1, ctypes.byref(out)), b"gf3_loading_create")
    refused(lib.gf3_loading_create(h, None, C, ctypes.byref(out)), b"gf3_loading_create")
    refused(lib.gf3_loading_create(h, as_p(good), C, None), b"gf3_loading_create")
    refused(lib.gf3_loading_create(None, as_p(good), C, ctypes.byref(out)), b"gf3_loading_create")
    assert lib.gf3_loading_bits(None) == 0 and lib.gf3_loading_bits(ld) == Bs
    lib.gf3_loading_destroy(None)
    for bad in (np.full(C, 3), np.zeros(C, dtype=int), np.full(C - 1, 2), np.full((2, C), 2), np.full(C, 2.0)):
        with pytest.raises(ValueError):
            eng.loading(bad)


# ---- end to end through the façade ------------------------------------------------------------------------------
# The gap.  G = 2 dB, chosen on the CPU with the restatement: symbol-level AWGN at this test's SNR profile (28 dB at bin
# 100 falling linearly to 2 dB at bin 1500), a QPSK probe of 3 packets of 8 symbols through noise_ref's estimate,
# bit_loading_from_snr on its per-carrier minimum, random codewords of the rate-1/2 code through loading_ref's mapper,
# estimate and noise-weighted demapper, decoded by ldpc_ref (50 iterations).  Failed codewords of 57 .. 79, noise as
# planted / raised by 2 dB / raised by 3 dB, three seeds each:  G = 0: 0 / 0 / 0,  G = 1: 0 / 0 / 0,  G = 2: 0 / 0 / 0,
# G = 3: 0 / 0 / 0,  G = 4: 0 / 0 / 0 (the minimum over three packets of a 16-sample estimate is itself conservative).
# Every G tried keeps the asked-for 2 dB; 2 dB is taken rather than 0 because the simulation has no channel estimate in
# it: four pilot symbols on each side add up to a quarter of the noise again (1 dB).  At G = 2 the simulated tables hold
# about 300 / 380 / 330 / 380 carriers of 0 / 2 / 4 / 6 bits, Bs about 4390 against 2 C = 2800.
GAP_DB = 2.0
SNR_ENDS = ((100, 1500), (28.0, 2.0))
A2 = dict(no_pilots=4, packet_length=8)
F_E2E = 3


def shaped_noise(n, seed):
    """White noise through an FFT mask: the noise density that puts the per-carrier SNR of a unit-energy constellation
    on the line SNR_ENDS (flat beyond its ends).  A data symbol's 4096-point transform holds 2 x the constellation point
    (|X|^2 = 4 at unit energy) and N g^2 of masked unit-variance noise."""
    rng = np.random.default_rng(seed)
    X = np.fft.rfft(rng.normal(0.0, 1.0, n))
    f = np.arange(len(X)) * 4096.0 / n                       # frequency in carrier units
    snr = np.interp(f, *SNR_ENDS)
    return np.fft.irfft(X * np.sqrt(4.0 / (4096.0 * 10 ** (snr / 10))), n)


def bodies(x, rx, F, lead):
    """[F * D, N] the data symbols' bodies (prefix removed) of a stream that transmit() made, `lead` samples in."""
    S, Nf, Pn, Dn = rx.ofdm_symbol_size + rx.cp_length, rx.ofdm_symbol_size, rx.no_pilots, rx.packet_length
    frame = rx.chirp_length + (2 * Pn + Dn) * S
    at = [lead + f * frame + rx.chirp_length + (Pn + l) * S + rx.cp_length for f in range(F) for l in range(Dn)]
    return np.stack([x[a: a + Nf] for a in at])


def send(encoding, order, payload, seed):
    """(transmitter, the bits its encode() put on the air, the stream with 2000 zeros on each side, even length)."""
    from gf3_audio_modem_amd.OFDM import receiver
    tx = receiver("A2", encoding=encoding, **A2)
    tx.bit_loading = order
    np.random.seed(seed)
    sent = np.asarray(tx.encode(payload))
    np.random.seed(seed)
    sig = tx.transmit(payload)
    sig = np.concatenate([np.zeros(2000), sig, np.zeros(2000 + len(sig) % 2)])
    return tx, sent, sig


def listen(encoding, order, stream, weighting="noise"):
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2", encoding=encoding, **A2)
    rx.bit_loading, rx.llr_weighting = order, weighting
    out, _, _ = rx.receive(stream)
    return rx, out


def test_facade_probe_allocation_and_loaded_round_trip():
    """Mode A2, "QCLDPC-1/2", 4 pilot and 8 data symbols per packet, 3 packets, noise whose density rises over the band
    so that the per-carrier SNR falls from 28 dB at bin 100 to 2 dB at bin 1500.  (a) a QPSK probe under
    llr_weighting = "noise" leaves last_snr_db; (b) bit_loading_from_snr(last_snr_db, GAP_DB) holds all four orders and
    more than 2 bits per carrier on average; (c) a fresh payload under that table, through a fresh noise draw, comes
    back exactly, every codeword converged; (d) the same with an all-6 table does not; (e) under "None" the raw bit
    error rate of the table's loaded carriers is below the rate of the same carriers under all-6 (read as: the table,
    not 64-QAM, is what the carriers hold; the carriers of order 6 alone carry 64-QAM in both runs and differ by the
    noise draw only -- their two rates are printed)."""
    from gf3_audio_modem_amd.loading import bit_loading_from_snr, loading_layout
    C, D, F = 1400, A2["packet_length"], F_E2E
    rng = np.random.default_rng(2027)
    # (a) the probe, and the construction of the noise on this test's own samples
    probe = rng.integers(0, 2, size=43 * 768)                # 43 codewords: three QPSK packets
    tx, _, sig = send("QCLDPC-1/2", None, probe, seed=11)
    assert tx.no_packets == F
    noise = shaped_noise(len(sig), seed=21)
    ps = (np.abs(np.fft.rfft(bodies(sig, tx, F, 2000), axis=1)) ** 2).mean(axis=0)[100:1500]
    pn = (np.abs(np.fft.rfft(bodies(noise, tx, F, 2000), axis=1)) ** 2).mean(axis=0)[100:1500]
    np.testing.assert_allclose(ps, 4.0, rtol=1e-9)           # QPSK: every carrier at unit energy
    planted = np.interp(np.arange(100, 1500), *SNR_ENDS)
    smooth = np.convolve(10 * np.log10(ps / pn), np.ones(50) / 50, mode="valid")
    line = np.convolve(planted, np.ones(50) / 50, mode="valid")
    print(f"planted SNR: smoothed measured - line in [{(smooth - line).min():.2f}, {(smooth - line).max():.2f}] dB; "
          f"ends {smooth[0]:.2f} .. {smooth[-1]:.2f} dB")
    assert np.abs(smooth - line).max() < 1.0 and smooth[0] > 26.0 and smooth[-1] < 4.0
    rx, _ = listen("QCLDPC-1/2", None, sig + noise)
    snr = rx.last_snr_db
    assert snr.shape == (F, C) and np.isfinite(snr).all()
    # (b) the allocation
    order = bit_loading_from_snr(snr, gap_db=GAP_DB)
    Bs, off = loading_layout(order)
    counts = {m: int((order == m).sum()) for m in (0, 2, 4, 6)}
    print(f"allocation at G = {GAP_DB} dB: carriers per order {counts}, Bs = {Bs}")
    assert all(counts.values()) and Bs > 2 * C
    # (c) the loaded round trip: a fresh payload, a fresh noise draw
    n_cw = F * D * Bs // 1536
    payload = rng.integers(0, 2, size=n_cw * 768)
    tx, _, sig = send("QCLDPC-1/2", order, payload, seed=12)
    assert tx.no_packets == F and tx.loaded_bits_per_symbol == Bs
    rx, out = listen("QCLDPC-1/2", order, sig + shaped_noise(len(sig), seed=22))
    rep = rx.last_decode_report
    print(f"loaded: {rep['codewords']} codewords, {rep['inner_failed']} failed; bit errors {int(np.sum(out[: len(payload)] != payload))}")
    assert rep["codewords"] == n_cw and rep["inner_failed"] == 0
    assert out.dtype == np.int64 and np.array_equal(out[: len(payload)], payload)
    assert rx.last_snr_db.shape == (F, C) and np.isfinite(rx.last_snr_db).all()          # carriers of order 0 included
    # (d) the control: 64-QAM everywhere, the same stream parameters
    all6 = np.full(C, 6, dtype=np.uint8)
    n6 = F * D * 6 * C // 1536
    pay6 = rng.integers(0, 2, size=n6 * 768)
    tx, _, sig6 = send("QCLDPC-1/2", all6, pay6, seed=13)
    assert tx.no_packets == F
    rx6, out6 = listen("QCLDPC-1/2", all6, sig6 + shaped_noise(len(sig6), seed=22))
    print(f"all-6: {rx6.last_decode_report['codewords']} codewords, {rx6.last_decode_report['inner_failed']} failed")
    assert rx6.last_decode_report["inner_failed"] > 0 and not np.array_equal(out6[: len(pay6)], pay6)
    # (e) raw bit error rates under "None"
    raw = rng.integers(0, 2, size=F * D * Bs)
    _, sent, s1 = send("None", order, raw, seed=14)
    assert np.array_equal(sent, raw)
    _, got = listen("None", order, s1 + shaped_noise(len(s1), seed=23), weighting="csi")
    assert got.dtype == np.int64 and got.shape == (F * D * Bs,)
    raw6 = rng.integers(0, 2, size=F * D * 6 * C)
    _, _, s2 = send("None", all6, raw6, seed=15)
    _, got6 = listen("None", all6, s2 + shaped_noise(len(s2), seed=23), weighting="csi")
    assert got6.shape == (F * D * 6 * C,)
    err = (got != raw).reshape(F * D, Bs)
    err6 = (got6 != raw6).reshape(F * D, C, 6)
    loaded, six = order > 0, order == 6
    ber = err.mean()
    ber6 = err6[:, loaded].mean()
    first6 = np.concatenate([err[:, off[c]: off[c] + 6].reshape(-1) for c in np.flatnonzero(six)]).mean()
    print(f"raw BER on the table's loaded carriers: {ber:.4f} under the table, {ber6:.4f} under all-6; "
          f"on its 6-bit carriers: {first6:.4f} under the table, {err6[:, six].mean():.4f} under all-6")
    assert ber < ber6
