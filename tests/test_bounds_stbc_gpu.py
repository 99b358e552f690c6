"""The two ABI entries of transmit diversity inside guard bands (tests/guarded.py): dressings A, B and plain, plain and skewed
by one element, bit-for-bit equal outputs and untouched bands.  This only compares bytes.

The rows are entered in the table of tests/test_bounds_signal_gpu.py (`BS.case`), which is the table the census of
tests/test_guarded_cpu.py reads, as tests/test_bounds_mimo_gpu.py enters its own: importing this module is what gives the
two entries their rows there, and they run here.  That module's geometry has an odd number of data symbols, which the code
refuses, so the context here is its geometry with D = 4 (and P = 2 for the cover)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import tables as T
from tests import test_bounds_signal_gpu as BS

pytestmark = pytest.mark.gpu
ENTRIES = ("gf3_stbc_slope", "gf3_stbc_detect")
c128, f64, f32 = torch.complex128, torch.float64, torch.float32
D = 4


@functools.lru_cache(maxsize=None)
def setup():
    from gf3_audio_modem_amd import _lib
    from tests.util import engine_for
    s = BS.Setup()
    s.p = T.params_for("qpsk_ref", BS.N, T.comb3(BS.N // 2 - 1), P=2, D=D, CP=BS.CP)
    s.eng = engine_for(s.p, in_dtype=f64)
    s.lib, s.h, s.stream, s.err = s.eng.lib, s.eng._h, s.eng._stream, _lib.last_error
    return s


def arrays(a, s, B, F, planted, spectra=True):
    """B branches of seeded estimates (and spectra) as `in_` arrays -> the pointer tables"""
    p = s.p
    rng = np.random.default_rng(B)
    cn = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    Ys, Hs = [], []
    for b in range(B):
        Y, H = cn(F * p.D, p.N // 2 + 1), cn(F, 2, 2, p.K)
        if planted and b == 0:
            Y[1, p.data_carriers[3]] = complex(np.nan, 1.0)
            H[F - 1, 1, 0, p.data_carriers[5] - 1] = complex(np.inf, 0.0)
        if spectra:
            Ys.append(a.in_(f"d_Y_c128[{b}]", Y))
        Hs.append(a.in_(f"d_H_c128[{b}]", H))
    tab = lambda xs: (C.c_void_p * B)(*[x.data_ptr() for x in xs])
    return (tab(Ys) if spectra else None), tab(Hs), rng


for B in (1, 2, 3, 4):
    for planted in ((False, True) if B == 2 else (False,)):
        for empty in ((False, True) if B == 2 and not planted else (False,)):
            label = f"B{B}{'-nonfinite' if planted else ''}{'-F0' if empty else ''}"

            @BS.case("gf3_stbc_slope", label)
            def _(a, B=B, planted=planted, empty=empty):
                s = setup()
                rows = BS.NF
                _, Ht, _ = arrays(a, s, B, rows, planted, spectra=False)
                slope = a.out("d_slope_f64", (rows,), f64)
                F = 0 if empty else rows
                BS.finish(a, s, s.lib.gf3_stbc_slope(s.h, B, Ht, F, BS.ptr(slope), s.stream()), F)

            @BS.case("gf3_stbc_detect", label)
            def _(a, B=B, planted=planted, empty=empty):
                s = setup()
                p, rows = s.p, BS.NF
                Yt, Ht, rng = arrays(a, s, B, rows, planted)
                slope = a.in_("d_slope_f64", 3e-3 * rng.normal(size=rows))
                llr = a.out("d_llr_f32", (rows, p.D, p.C, p.mu), f32)
                F = 0 if empty else rows
                BS.finish(a, s, s.lib.gf3_stbc_detect(s.h, B, Yt, Ht, BS.ptr(slope), F, BS.ptr(llr), s.stream()), F)


ROWS = [(name, i) for name in ENTRIES for i in range(len(BS.CASES[name]))]


@pytest.mark.parametrize("name, i", ROWS, ids=[f"{name}-{BS.CASES[name][i][0]}" for name, i in ROWS])
def test_bounds(name, i):
    G.run(BS.CASES[name][i][1], device="cuda")
