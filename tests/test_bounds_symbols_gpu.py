"""The symbol-domain ABI entries inside guard bands (tests/guarded.py): everything that takes equalised symbols, spectra or
bits -- gf3_equalise, the demappers, the noise estimators and their weighted demappers, the interleaver, the loaded pair,
gf3_combine_branches, gf3_track_phase, gf3_feedback_equalise, gf3_unpack_bits.  This only compares bytes; the values are
held by the test_*_gpu.py files of each stage.

The rows are entered in the table of tests/test_bounds_signal_gpu.py (`BS.case`), which the census of
tests/test_guarded_cpu.py reads, and run here (ENTRIES).  No row needs a stream: an engine and seeded arrays are enough.
Symbols are table points plus a little seeded noise, so that every decision is far from a tie.

Geometries (three packets each):
    base   N = 1024, comb3 (C = 171, odd, not contiguous), D = 3: the geometry of the signal file
    tall   the same map with D = 11: the 8-strided symbol loops of the noise estimators run twice for w = 0 .. 2 and once
           for w = 3 .. 7; the feedback kernel has a full row tile of 8 and a partial one of 3, and a `half_symbols`
           window that crosses the tile edge
    wide   N = 2048, carriers 1 .. 600, D = 3: C > 512 gives 88 threads of track_phase_kernel a second carrier, C > 256
           gives the 256-thread demappers a third pass of 88, 600 = 4 x 128 + 88 a partial feedback tile, 600 = 9 x 64 + 24
           a partial lane column in noise_estimate_cs_kernel; D C mu = 3600 gives the interleaver a second, partial block
    broad  N = 4096, carriers 1 .. 1100, D = 3, for two kernels only: noise_estimate_cs_kernel then holds 9 columns a half
           (its instantiation of 12, which loads them four at a time), track_phase_kernel three carriers a thread
Not-written ranges: none inside an accepted call (every element of every output is promised); a refusal and F == 0 write
nothing.  gf3_unpack_bits' output is 16-byte aligned and gf3_soft_demap_loaded's LLRs 8-byte aligned, as the header
demands."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import loading_ref as LR
from tests import tables as T
from tests import test_bounds_signal_gpu as BS

pytestmark = pytest.mark.gpu
ENTRIES = ("gf3_equalise", "gf3_demap_hard", "gf3_soft_demap", "gf3_soft_demap_csi", "gf3_noise_estimate", "gf3_soft_demap_nw",
           "gf3_noise_estimate_cs", "gf3_soft_demap_nw_cs", "gf3_interleave", "gf3_noise_estimate_loaded",
           "gf3_soft_demap_loaded", "gf3_combine_branches", "gf3_track_phase", "gf3_feedback_equalise", "gf3_unpack_bits")
c128, f64, f32, i64, i32, i16, u8 = (torch.complex128, torch.float64, torch.float32, torch.int64, torch.int32, torch.int16,
                                     torch.uint8)
F = BS.NF
EINVAL = -1
GEOMS = dict(base=(1024, lambda K: T.comb3(K), 3), tall=(1024, lambda K: T.comb3(K), 11),
             wide=(2048, lambda K: np.arange(1, 601), 3), broad=(4096, lambda K: np.arange(1, 1101), 3))
ptr = BS.ptr


@functools.lru_cache(maxsize=None)
def setup(geom="base", table="qpsk_ref", P=1):
    """An engine of the geometry (no stream) with the names the BS helpers use."""
    from gf3_audio_modem_amd import _lib
    from tests.util import engine_for
    N, carriers, D = GEOMS[geom]
    s = BS.Setup()
    s.p = T.params_for(table, N, carriers(N // 2 - 1), P=P, D=D, CP=BS.CP)
    s.eng = engine_for(s.p)
    s.lib, s.h, s.stream, s.bpf, s.err = s.eng.lib, s.eng._h, s.eng._stream, s.eng.bytes_per_frame, _lib.last_error
    s.nbp = s.p.D * s.p.C * s.p.mu
    return s


def cn(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def symbols(points, shape, seed, planted=False):
    """Seeded table points plus noise of 0.02 a part (the closest boundary of any table here is 0.15 away); planted: a NaN
    part in the second row and an infinite one in the last element."""
    rng = np.random.default_rng(seed)
    eq = np.asarray(points)[rng.integers(0, len(points), shape)] + 0.02 * cn(rng, *shape)
    if planted:
        eq[1, 3] = complex(np.nan, 1.0)
        eq[-1, -1] = complex(np.inf, 0.0)
    return eq


def eq_of(s, seed=1, planted=False):
    return symbols(s.p.const_points, (F * s.p.D, s.p.C), seed, planted)


def variances(s, seed, planted=False, cols=None):
    """Positive seeded variances [F, cols]; planted: a NaN, an Inf and a zero, and a packet whose variances are all zero."""
    rng = np.random.default_rng(seed)
    v = 1e-3 * (0.5 + rng.random((F, s.p.C if cols is None else cols)))
    if planted:
        v[0, 0], v[0, 1], v[0, 2] = np.nan, np.inf, 0.0
        v[1, :] = 0.0
    return v


def first_variant(it):
    """(item, empty) over `it`, with one more F == 0 run of the first item"""
    for k, x in enumerate(it):
        yield x, False
        if k == 0:
            yield x, True


# ---- gf3_equalise: spectra in, the demodulator's dumps out ------------------------------------------------------------------------
EQUALISE_RUNS = [("base", P, tb, d) for P in (1, 2) for tb in ("qpsk_ref", "rect8") for d in (True, False)]
EQUALISE_RUNS += [("wide", 1, "qpsk_ref", True)]                # (the N = 2048 kernel on a contiguous map)
for (geom, P, tb, dumped), empty in first_variant(EQUALISE_RUNS):
    @BS.case("gf3_equalise", f"{geom}-P{P}-{tb}-{'dumps' if dumped else 'bare'}{'-F0' if empty else ''}")
    def _(a, geom=geom, P=P, tb=tb, dumped=dumped, empty=empty):
        s = setup(geom, tb, P)
        p = s.p
        rng = np.random.default_rng(P)
        k = np.arange(1, p.K + 1)
        H = (1.0 + 0.3 * np.cos(k / 40.0)) * np.exp(-2j * np.pi * k * 1.5 / p.N)
        known = p.known_symbols()
        X = np.tile(T.QPSK_FILL[rng.integers(0, 4, p.K)], (F, p.D, 1))
        X[:, :, p.data_carriers - 1] = eq_of(s).reshape(F, p.D, p.C)
        pilots = lambda: np.tile(H * known, (F, P, 1)) + 1e-3 * cn(rng, F, P, p.K)
        data, start, end = a.in_("d_data", H * X), a.in_("d_start", pilots()), a.in_("d_end", pilots())
        eq_all = a.out("d_eq_all", (F * p.D, p.K), c128)
        o = BS.dumps(a, s, F, np.zeros(F, dtype=bool), [n for n in BS.ALL_DUMPS if n != "eq"] if dumped else ())
        bits = a.out("d_bits", (F, s.bpf), u8)
        n = 0 if empty else F
        BS.finish(a, s, s.lib.gf3_equalise(s.h, ptr(data), ptr(start), ptr(end), n, ptr(eq_all), ptr(o["Hs"]), ptr(o["He"]),
                                           ptr(o["slope"]), ptr(o["Hest"]), ptr(bits), s.stream()), n)


# ---- the flat demappers: n symbols, any n ------------------------------------------------------------------------------------------
DEMAP_TABLES = ("qpsk_ref", "rect8", "psk8", "qam64")           # the bin kernel, the sep kernel at mu = 3, the literal scan, 8 x 8
for (tb, n, with_idx), empty in first_variant([(tb, n, w) for tb in DEMAP_TABLES for n in (1, 513, 1021) for w in (True, False)]):
    @BS.case("gf3_demap_hard", f"{tb}-n{n}{'-idx' if with_idx else ''}{'-n0' if empty else ''}")
    def _(a, tb=tb, n=n, with_idx=with_idx, empty=empty):
        s = setup("base", tb)
        sym = a.in_("d_sym_c128", symbols(s.p.const_points, (n,), n))
        bits = a.out("d_bits_u8", (n * s.p.mu,), u8)
        idx = a.out("d_idx_u8", (n,), u8) if with_idx else None
        m = 0 if empty else n
        BS.finish(a, s, s.lib.gf3_demap_hard(s.h, ptr(sym), m, ptr(bits), ptr(idx), s.stream()), m)

# (qam16_scaled_axes: mu = 4, the LLRs of a symbol stored four at a time)
for (tb, n), empty in first_variant([(tb, n) for tb in DEMAP_TABLES + ("qam16_scaled_axes",) for n in (1, 513, 1021)]):
    @BS.case("gf3_soft_demap", f"{tb}-n{n}{'-n0' if empty else ''}")
    def _(a, tb=tb, n=n, empty=empty):
        s = setup("base", tb)
        sym = a.in_("d_sym_c128", symbols(s.p.const_points, (n,), n))
        llr = a.out("d_llr_f32", (n * s.p.mu,), f32)
        m = 0 if empty else n
        BS.finish(a, s, s.lib.gf3_soft_demap(s.h, ptr(sym), m, 0.5, ptr(llr), s.stream()), m)

for (geom, tb), empty in first_variant([("base", "qpsk_ref"), ("base", "rect8"), ("wide", "qpsk_ref")]):
    @BS.case("gf3_soft_demap_csi", f"{geom}-{tb}{'-F0' if empty else ''}")
    def _(a, geom=geom, tb=tb, empty=empty):
        s = setup(geom, tb)
        p, rng = s.p, np.random.default_rng(3)
        eq, Hs, He = a.in_("d_eq_c128", eq_of(s)), a.in_("d_Hs_c128", cn(rng, F, p.K)), a.in_("d_He_c128", cn(rng, F, p.K))
        llr = a.out("d_llr_f32", (F * s.nbp,), f32)
        n = 0 if empty else F
        BS.finish(a, s, s.lib.gf3_soft_demap_csi(s.h, ptr(eq), ptr(Hs), ptr(He), n, ptr(llr), s.stream()), n)


# ---- the noise pair and its carrier x symbol form --------------------------------------------------------------------------------
NOISE_RUNS = [("base", "qpsk_ref", False), ("tall", "qpsk_ref", False), ("wide", "qpsk_ref", False), ("base", "rect8", False),
              ("base", "qpsk_ref", True), ("tall", "rect8", True), ("base", "qam64", False)]      # (qam64: six LLRs a symbol, stored in pairs)
for (geom, tb, planted), empty in first_variant(NOISE_RUNS):
    label = f"{geom}-{tb}{'-nonfinite' if planted else ''}{'-F0' if empty else ''}"

    @BS.case("gf3_noise_estimate", label)
    def _(a, geom=geom, tb=tb, planted=planted, empty=empty):
        s = setup(geom, tb)
        eq = a.in_("d_eq_c128", eq_of(s, 2, planted))
        var = a.out("d_var_f64", (F, s.p.C), f64)
        n = 0 if empty else F
        BS.finish(a, s, s.lib.gf3_noise_estimate(s.h, ptr(eq), n, ptr(var), s.stream()), n)
        if n and planted:                                       # "a NaN / Inf symbol makes v[f, c] non-finite"
            assert not torch.isfinite(var[0, 3]) and not torch.isfinite(var[F - 1, s.p.C - 1]) and torch.isfinite(var[0, 0])

    @BS.case("gf3_soft_demap_nw", label)
    def _(a, geom=geom, tb=tb, planted=planted, empty=empty):
        s = setup(geom, tb)
        eq, var = a.in_("d_eq_c128", eq_of(s, 2, planted)), a.in_("d_var_f64", variances(s, 4, planted))
        llr = a.out("d_llr_f32", (F, s.p.D, s.p.C, s.p.mu), f32)
        n = 0 if empty else F
        BS.finish(a, s, s.lib.gf3_soft_demap_nw(s.h, ptr(eq), ptr(var), n, ptr(llr), s.stream()), n)
        if n and planted:                                       # "w = 0 where v[f, c] is not finite (the LLR is then +0 ...)"
            assert not llr[0, :, :2].view(torch.int32).any() and llr[0, :, 2].any()

    @BS.case("gf3_noise_estimate_cs", label)
    def _(a, geom=geom, tb=tb, planted=planted, empty=empty):
        s = setup(geom, tb)
        eq = a.in_("d_eq_c128", eq_of(s, 2, planted))
        var_c, var_s = a.out("d_var_c_f64", (F, s.p.C), f64), a.out("d_var_s_f64", (F, s.p.D), f64)
        n = 0 if empty else F
        BS.finish(a, s, s.lib.gf3_noise_estimate_cs(s.h, ptr(eq), n, ptr(var_c), ptr(var_s), s.stream()), n)
        if n and planted:
            assert not torch.isfinite(var_c[0, 3]) and not torch.isfinite(var_s[0, 1]) and torch.isfinite(var_s[0, 0])

    for deint in (0, 1):
        @BS.case("gf3_soft_demap_nw_cs", f"{label}-deint{deint}")
        def _(a, geom=geom, tb=tb, planted=planted, empty=empty, deint=deint):
            s = setup(geom, tb)
            eq, var_c = a.in_("d_eq_c128", eq_of(s, 2, planted)), a.in_("d_var_c_f64", variances(s, 4, planted))
            var_s = a.in_("d_var_s_f64", variances(s, 5, planted, cols=s.p.D))
            llr = a.out("d_llr_f32", (F * s.nbp,), f32)
            n = 0 if empty else F
            BS.finish(a, s, s.lib.gf3_soft_demap_nw_cs(s.h, ptr(eq), ptr(var_c), ptr(var_s), n, deint, ptr(llr), s.stream()), n)


@BS.case("gf3_noise_estimate_cs", "broad-qpsk_ref")
def _(a):                                                           # 18 columns of 64 carriers: the instantiation of 12 a half
    s = setup("broad", "qpsk_ref")
    eq = a.in_("d_eq_c128", eq_of(s, 2))
    var_c, var_s = a.out("d_var_c_f64", (F, s.p.C), f64), a.out("d_var_s_f64", (F, s.p.D), f64)
    BS.finish(a, s, s.lib.gf3_noise_estimate_cs(s.h, ptr(eq), F, ptr(var_c), ptr(var_s), s.stream()), F)


# ---- gf3_interleave: nbp = 1026 (QPSK) and 1539 (rect8, odd); 3762 and 3600: a second block of 2048 elements, partial -------------
INTERLEAVE_RUNS = [("base", tb, eb, inv) for tb in ("qpsk_ref", "rect8") for eb in (1, 4) for inv in (0, 1)]
INTERLEAVE_RUNS += [("tall", "qpsk_ref", 1, 0), ("tall", "qpsk_ref", 4, 1), ("wide", "qpsk_ref", 4, 0), ("wide", "qpsk_ref", 1, 1)]
for (geom, tb, eb, inverse), empty in first_variant(INTERLEAVE_RUNS):
    @BS.case("gf3_interleave", f"{geom}-{tb}-bytes{eb}-inverse{inverse}{'-F0' if empty else ''}")
    def _(a, geom=geom, tb=tb, eb=eb, inverse=inverse, empty=empty):
        s = setup(geom, tb)
        x = np.random.default_rng(eb).integers(0, 200, (F, s.nbp)).astype(np.uint8 if eb == 1 else np.int32)
        d_in = a.in_("d_in", x)
        out = a.out("d_out", (F, s.nbp), u8 if eb == 1 else i32)
        n = 0 if empty else F
        BS.finish(a, s, s.lib.gf3_interleave(s.h, ptr(d_in), ptr(out), n, eb, inverse, s.stream()), n)


@BS.case("gf3_interleave", "qpsk_ref-bytes2-refused")
def _(a):                                                           # "arrays of 1- or 4-byte elements"; a refusal writes nothing
    s = setup("base", "qpsk_ref")
    d_in = a.in_("d_in", np.arange(F * s.nbp, dtype=np.int16).reshape(F, s.nbp))
    out = a.out("d_out", (F, s.nbp), i16)
    BS.finish(a, s, s.lib.gf3_interleave(s.h, ptr(d_in), ptr(out), F, 2, 0, s.stream()), F, want=EINVAL)


# ---- the loaded pair ---------------------------------------------------------------------------------------------------------------
def orders(Cn):
    """0 / 2 / 4 / 6 mixed.  `ends-0-6`: the first carrier carries nothing, the last six bits; `last-0`: the last carrier
    carries nothing, so the last LLR of a row belongs to the carrier before it."""
    mixed = np.array([0, 2, 4, 6], dtype=np.uint8)[np.arange(Cn) % 4]
    a, b = mixed.copy(), mixed.copy()
    a[0], a[-1] = 0, 6
    b[0], b[-1] = 4, 0
    return {"ends-0-6": a, "last-0": b}


@functools.lru_cache(maxsize=None)
def loaded(geom, which):
    """(setup, the loading -- made once, kept and destroyed by the engine --, Bs, symbols of each carrier's own table)"""
    s = setup(geom, "qpsk_ref", 2)
    order = orders(s.p.C)[which]
    ld = s.eng.loading(order)
    Bs, _ = LR.layout(order)
    known = s.p.known_symbols()[s.p.data_carriers - 1]
    rng = np.random.default_rng(len(which))
    clean = np.asarray(LR.map_loaded(rng.integers(0, 2, F * s.p.D * Bs), order, known)).reshape(F * s.p.D, s.p.C)
    return s, ld, Bs, clean + 0.02 * cn(rng, *clean.shape)


LOADED_RUNS = [("base", "ends-0-6"), ("base", "last-0"), ("wide", "ends-0-6"), ("wide", "last-0"), ("tall", "ends-0-6")]
for (geom, which), empty in first_variant(LOADED_RUNS):
    @BS.case("gf3_noise_estimate_loaded", f"{geom}-{which}{'-F0' if empty else ''}")
    def _(a, geom=geom, which=which, empty=empty):
        s, ld, Bs, eq0 = loaded(geom, which)
        eq = a.in_("d_eq_c128", eq0)
        var = a.out("d_var_f64", (F, s.p.C), f64)
        n = 0 if empty else F
        BS.finish(a, s, s.lib.gf3_noise_estimate_loaded(s.h, ld.handle, ptr(eq), n, ptr(var), s.stream()), n)

    for weight in ("unit", "var", "csi") + (("var+csi", "Hs-only") if geom == "base" and not empty else ()):
        @BS.case("gf3_soft_demap_loaded", f"{geom}-{which}-{weight}{'-F0' if empty else ''}")
        def _(a, geom=geom, which=which, empty=empty, weight=weight):
            s, ld, Bs, eq0 = loaded(geom, which)
            rng = np.random.default_rng(9)
            eq = a.in_("d_eq_c128", eq0)
            Hs = a.in_("d_Hs_c128", cn(rng, F, s.p.K)) if weight in ("csi", "var+csi", "Hs-only") else None
            He = a.in_("d_He_c128", cn(rng, F, s.p.K)) if weight in ("csi", "var+csi") else None
            var = a.in_("d_var_f64", variances(s, 6, planted=which == "last-0")) if weight in ("var", "var+csi") else None
            llr = a.out("d_llr_f32", (F * s.p.D * Bs,), f32, align=8)            # "d_llr_f32 must be 8-byte aligned"
            n = 0 if empty else F
            BS.finish(a, s, s.lib.gf3_soft_demap_loaded(s.h, ld.handle, ptr(eq), ptr(Hs), ptr(He), ptr(var), n, ptr(llr), s.stream()),
                      n, want=EINVAL if weight in ("var+csi", "Hs-only") else 0)


# ---- gf3_combine_branches ----------------------------------------------------------------------------------------------------------
def branches(a, s, B, noise, planted):
    """The pointer tables of B branches (the detect_arrays idiom); the tables of the mode that is not read are NULL."""
    p, rng = s.p, np.random.default_rng(B)
    tab = lambda xs: (C.c_void_p * B)(*[x.data_ptr() for x in xs])
    eqs, Hss, Hes, vs = [], [], [], []
    for b in range(B):
        eqs.append(a.in_(f"d_eq_c128[{b}]", eq_of(s, 10 + b, planted and b == 0)))
        if noise:
            vs.append(a.in_(f"d_var_f64[{b}]", variances(s, 20 + b, planted and b == B - 1)))
        else:
            Hs, He = cn(rng, F, p.K), cn(rng, F, p.K)
            if planted and b == B - 1:
                Hs[0, p.data_carriers[5] - 1] = complex(np.nan, 0.0)
                He[F - 1, p.data_carriers[7] - 1] = complex(0.0, np.inf)
            Hss.append(a.in_(f"d_Hs_c128[{b}]", Hs))
            Hes.append(a.in_(f"d_He_c128[{b}]", He))
    return tab(eqs), (None if noise else tab(Hss)), (None if noise else tab(Hes)), (tab(vs) if noise else None)


COMBINE_OUTS = (("eq",), ("wsum",), ("llr",), ("eq", "wsum", "llr"))
COMBINE_RUNS = [("base", "qpsk_ref", B, mode, outs, False) for B in (1, 2, 3, 4) for mode in (0, 1) for outs in COMBINE_OUTS]
COMBINE_RUNS += [(geom, tb, 2, mode, COMBINE_OUTS[3], planted) for mode in (0, 1)
                 for geom, tb, planted in (("base", "qpsk_ref", True), ("wide", "qpsk_ref", False), ("base", "rect8", False),
                                             ("tall", "qam64", False))]
for (geom, tb, B, mode, outs, planted), empty in first_variant(COMBINE_RUNS):
    @BS.case("gf3_combine_branches", f"{geom}-{tb}-B{B}-{'noise' if mode else 'csi'}-{'+'.join(outs)}{'-nonfinite' if planted else ''}"
                                     f"{'-F0' if empty else ''}")
    def _(a, geom=geom, tb=tb, B=B, mode=mode, outs=outs, planted=planted, empty=empty):
        s = setup(geom, tb, 2)
        p = s.p
        eqt, Hst, Het, vt = branches(a, s, B, mode == 1, planted)
        eq_out = a.out("d_eq_out_c128", (F * p.D, p.C), c128) if "eq" in outs else None
        wsum = a.out("d_wsum_f64", (F * p.D, p.C), f64) if "wsum" in outs else None
        llr = a.out("d_llr_f32", (F * s.nbp,), f32) if "llr" in outs else None
        n = 0 if empty else F
        BS.finish(a, s, s.lib.gf3_combine_branches(s.h, B, eqt, mode, Hst, Het, vt, n, ptr(eq_out), ptr(wsum), ptr(llr), s.stream()), n)


# ---- gf3_track_phase ---------------------------------------------------------------------------------------------------------------
for (geom, in_place, extras), empty in first_variant([(g, ip, ex) for g in GEOMS for ip in (False, True) for ex in (True, False)
                                                      if g != "broad" or ip == ex]):
    @BS.case("gf3_track_phase", f"{geom}-{'inplace' if in_place else 'outofplace'}{'-phase-measured' if extras else ''}"
                                f"{'-F0' if empty else ''}")
    def _(a, geom=geom, in_place=in_place, extras=extras, empty=empty):
        s = setup(geom, "qpsk_ref")
        p = s.p
        # a phase that drifts over the packet's symbols, and a non-finite symbol ("is left out")
        eq0 = eq_of(s, 7, planted=True) * np.exp(1j * 0.03 * (np.arange(F * p.D) % p.D))[:, None]
        if in_place:                                            # "d_out == d_eq is allowed (in place)"
            eq = out = a.inout("d_eq_c128", eq0)
        else:
            eq, out = a.in_("d_eq_c128", eq0), a.out("d_out_c128", (F * p.D, p.C), c128)
        phase = a.out("d_phase_f64", (F, p.D, 2), f64) if extras else None
        meas = a.out("d_measured", (F, p.D), u8) if extras else None
        n = 0 if empty else F
        BS.finish(a, s, s.lib.gf3_track_phase(s.h, ptr(eq), n, ptr(out), ptr(phase), ptr(meas), s.stream()), n)
        if n and extras:
            assert int(meas.max()) <= 1                         # "d_measured [F, D] = 0 / 1"


# ---- gf3_feedback_equalise ---------------------------------------------------------------------------------------------------------
def feedback_planes(s, mask):
    """bits [F, D C mu] of the symbols eq_of(s, 8) was made from (its decisions), and the known mask: `all`, `clear`, or one
    codeword's worth of C mu bits from bit 100 of every packet (it ends inside a symbol)."""
    p = s.p
    eq = eq_of(s, 8, planted=True)
    idx = np.abs(np.nan_to_num(eq, nan=0.0, posinf=0.0)[:, :, None] - p.const_points).argmin(axis=2)
    bits = p.const_bits[idx].reshape(F, s.nbp).astype(np.uint8)
    known = np.zeros((F, s.nbp), dtype=np.uint8)
    if mask == "all":
        known[:] = 1
    elif mask == "codeword":
        known[:, 100: 100 + p.C * p.mu] = 0xFF                  # (non-zero = 1)
    return eq, bits, known


FEEDBACK_RUNS = [(g, w, m, m != "clear") for g in ("base", "tall", "wide") for w in ((0, 0), (2, 8), (8, 64)) for m in ("all", "clear", "codeword")]
FEEDBACK_RUNS += [("base", (2, 8), "codeword", False), ("base", (8, 64), "codeword", "refused")]
for (geom, (hs, hb), mask, gain), empty in first_variant(FEEDBACK_RUNS):
    @BS.case("gf3_feedback_equalise", f"{geom}-w{hs}x{hb}-{mask}{'-refused' if gain == 'refused' else '-gain' if gain else ''}"
                                      f"{'-F0' if empty else ''}")
    def _(a, geom=geom, hs=hs, hb=hb, mask=mask, gain=gain, empty=empty):
        s = setup(geom, "rect8" if geom == "tall" else "qpsk_ref")           # (mu = 3: labels byte by byte; mu = 2: two at a time)
        p = s.p
        eq0, bits0, known0 = feedback_planes(s, mask)
        eq, bits, known = a.in_("d_eq_c128", eq0), a.in_("d_bits_u8", bits0), a.in_("d_known_u8", known0)
        g = a.out("d_gain_c128", (F * p.D, p.C), c128) if gain else None
        n = 0 if empty else F
        if gain == "refused":                                   # "d_out must not be d_eq": GF3_EINVAL, nothing written
            rc = s.lib.gf3_feedback_equalise(s.h, ptr(eq), ptr(bits), ptr(known), n, hs, hb, 3, ptr(eq), ptr(g), None, 0, s.stream())
            return BS.finish(a, s, rc, n, want=EINVAL)
        out = a.out("d_out_c128", (F * p.D, p.C), c128)
        BS.finish(a, s, s.lib.gf3_feedback_equalise(s.h, ptr(eq), ptr(bits), ptr(known), n, hs, hb, 3, ptr(out), ptr(g), None, 0,
                                                    s.stream()), n)


# ---- gf3_unpack_bits: F D C mu = 3078 (QPSK, even) and 4617 (rect8, odd: the last element takes the scalar store) -----------------
UNPACK_RUNS = [("base", tb, m) for tb in ("qpsk_ref", "rect8") for m in ("nomask", "Cmu", "seven")] + [("wide", "qpsk_ref", "seven")]
for (geom, tb, mask), empty in first_variant(UNPACK_RUNS):
    @BS.case("gf3_unpack_bits", f"{geom}-{tb}-{mask}{'-F0' if empty else ''}")
    def _(a, geom=geom, tb=tb, mask=mask, empty=empty):
        s = setup(geom, tb)
        rng = np.random.default_rng(11)
        packed = a.in_("d_bits_packed", rng.integers(0, 256, (F, s.bpf)).astype(np.uint8))
        n_mask = dict(nomask=0, Cmu=s.p.C * s.p.mu, seven=7)[mask]
        d_mask = a.in_("d_mask_u8", rng.integers(0, 2, n_mask).astype(np.uint8)) if n_mask else None
        out = a.out("out_i64", (F * s.nbp,), i64, align=16)      # "16 bytes per lane": the one-int64 skew would be refused
        n = 0 if empty else F
        BS.finish(a, s, s.lib.gf3_unpack_bits(s.h, ptr(packed), n, ptr(d_mask), n_mask, ptr(out), s.stream()), n)
        if n:
            assert int(out.max()) <= 1 and int(out.min()) >= 0


ROWS = [(name, i) for name in ENTRIES for i in range(len(BS.CASES[name]))]


@pytest.mark.parametrize("name, i", ROWS, ids=[f"{name}-{BS.CASES[name][i][0]}" for name, i in ROWS])
def test_bounds(name, i):
    G.run(BS.CASES[name][i][1], device="cuda")
