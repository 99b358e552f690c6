"""The two ABI entries of 2 x 2 spatial multiplexing inside guard bands (tests/guarded.py): dressings A, B and plain, plain
and skewed by one element, bit-for-bit equal outputs and untouched bands.  This only compares bytes.

The rows are written with the helpers of tests/test_bounds_signal_gpu.py -- its geometry, its streams in every sample
storage, its placements of packets at both ends of the samples -- and are entered in ITS table (`BS.case`), which is the
table the census of tests/test_guarded_cpu.py reads: importing this module is what gives the two entries their rows there.
`BS.ROWS` was made when that module was imported, so its own `test_bounds` does not run them a second time; they run here."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import test_bounds_signal_gpu as BS

pytestmark = pytest.mark.gpu
ENTRIES = ("gf3_mimo_pilots", "gf3_mimo_detect")
c128, f64, f32, i32 = torch.complex128, torch.float64, torch.float32, torch.int32

for st in BS.STORAGES:
    for P in ((2, 4) if st == "f64" else (2,)):
        for empty in ((False, True) if (st, P) == ("f64", 2) else (False,)):
            @BS.case("gf3_mimo_pilots", f"{st}-P{P}{'-F0' if empty else ''}")
            def _(a, st=st, P=P, empty=empty):
                s = BS.setup(st, "qpsk_ref", P)
                x, off, F, rows, ragged = BS.frames_in(a, s, empty)
                H = a.out("d_H_out_c128", (rows, 2, 2, s.p.K), c128)
                status = a.out("d_status_i32", (rows,), i32)
                BS.finish(a, s, s.lib.gf3_mimo_pilots(s.h, BS.ptr(x), x.numel(), BS.ptr(off), F, BS.ptr(H), BS.ptr(status), s.stream()), F)
                if F:                                               # a ragged packet: status 1 and NaN rows, written
                    assert status.tolist() == ragged.astype(int).tolist()
                    bad = torch.from_numpy(ragged).to(H.device)
                    assert torch.isnan(H[bad].real).all() and torch.isnan(H[bad].imag).all() and torch.isfinite(H[~bad].real).all()


def detect_arrays(a, s, B, F, planted):
    """B branches of seeded spectra, estimates and slopes as `in_` arrays -> the three pointer tables and the tensors"""
    p = s.p
    rng = np.random.default_rng(B)
    cn = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    Ys, Hs, Ss = [], [], []
    for b in range(B):
        Y, H = cn(F * p.D, p.N // 2 + 1), cn(F, 2, 2, p.K)
        if planted and b == 0:
            Y[1, p.data_carriers[3]] = complex(np.nan, 1.0)
            H[F - 1, 1, 0, p.data_carriers[5] - 1] = complex(np.inf, 0.0)
        Ys.append(a.in_(f"d_Y_c128[{b}]", Y))
        Hs.append(a.in_(f"d_H_c128[{b}]", H))
        Ss.append(a.in_(f"d_slope_f64[{b}]", 3e-3 * rng.normal(size=F)))
    tab = lambda xs: (C.c_void_p * B)(*[x.data_ptr() for x in xs])
    return tab(Ys), tab(Hs), tab(Ss)


for B in (1, 2, 3, 4):
    for planted in ((False, True) if B == 2 else (False,)):
        for empty in ((False, True) if B == 2 and not planted else (False,)):
            @BS.case("gf3_mimo_detect", f"B{B}{'-nonfinite' if planted else ''}{'-F0' if empty else ''}")
            def _(a, B=B, planted=planted, empty=empty):
                s = BS.setup("f64", "qpsk_ref", 2)
                p, rows = s.p, BS.NF
                Yt, Ht, St = detect_arrays(a, s, B, rows, planted)
                llr = a.out("d_llr_f32", (rows, 2, p.D, p.C, p.mu), f32)
                F = 0 if empty else rows
                BS.finish(a, s, s.lib.gf3_mimo_detect(s.h, B, Yt, Ht, St, F, BS.ptr(llr), s.stream()), F)


ROWS = [(name, i) for name in ENTRIES for i in range(len(BS.CASES[name]))]


@pytest.mark.parametrize("name, i", ROWS, ids=[f"{name}-{BS.CASES[name][i][0]}" for name, i in ROWS])
def test_bounds(name, i):
    G.run(BS.CASES[name][i][1], device="cuda")
