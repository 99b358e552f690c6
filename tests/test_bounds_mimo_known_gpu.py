"""gf3_mimo_detect_known inside guard bands (tests/guarded.py): dressings A, B and plain, plain and skewed by one element --
for the two byte planes one BYTE, so that the kernel's 2-byte reads of them start at odd addresses --, bit-for-bit equal
outputs and untouched bands.  This only compares bytes.

The rows are entered in the table of tests/test_bounds_signal_gpu.py (`BS.case`), which is the table the census of
tests/test_guarded_cpu.py reads, as tests/test_bounds_mimo_gpu.py enters its own: importing this module is what gives the
entry its rows there, and they run here.  Geometry and branches are that module's (`detect_arrays`): N = 1024, CP = 32, the
carrier map comb3 (C = 171: one partial 256-carrier tile), D = 3, three packet pairs."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import test_bounds_signal_gpu as BS
from tests.test_bounds_mimo_gpu import detect_arrays

pytestmark = pytest.mark.gpu
ENTRIES = ("gf3_mimo_detect_known",)
f32 = torch.float32


def plane_arrays(a, p, F, seed):
    """The two byte planes [F][2][D][C][mu] as `in_` arrays: seeded bits, a third of them known, some bytes other than 0 / 1"""
    rng = np.random.default_rng(seed)
    shape = (F, 2, p.D, p.C, p.mu)
    bits = rng.integers(0, 2, size=shape).astype(np.uint8) * rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=shape)
    known = (rng.random(size=shape) < 1 / 3).astype(np.uint8) * rng.choice(np.array([1, 128, 255], dtype=np.uint8), size=shape)
    return a.in_("d_bits_u8", bits), a.in_("d_known_u8", known)


for B in (1, 2, 3, 4):
    for kind in (("plain", "nonfinite", "weighted", "F0") if B == 2 else ("plain",)):
        @BS.case("gf3_mimo_detect_known", f"B{B}{'' if kind == 'plain' else '-' + kind}")
        def _(a, B=B, kind=kind):
            s = BS.setup("f64", "qpsk_ref", 2)
            p, rows = s.p, BS.NF
            Yt, Ht, St = detect_arrays(a, s, B, rows, kind == "nonfinite")
            bits, known = plane_arrays(a, p, rows, 40 + B)
            w = None
            if kind == "weighted":
                wv = np.exp(np.random.default_rng(B).normal(size=(B, rows, p.C)))
                wv[0, 0, 7], wv[:, rows - 1, 9], wv[B - 1, 0, 11] = 0.0, 0.0, np.nan
                w = a.in_("d_w_f64", wv)
            llr = a.out("d_llr_f32", (rows, 2, p.D, p.C, p.mu), f32)
            F = 0 if kind == "F0" else rows
            BS.finish(a, s, s.lib.gf3_mimo_detect_known(s.h, B, Yt, Ht, St, BS.ptr(w), BS.ptr(bits), BS.ptr(known), F, BS.ptr(llr),
                                                        s.stream()), F)
            if F:
                assert torch.isfinite(llr).all()
                assert ((llr.abs() == 1e30) == (known != 0)).all()


ROWS = [(name, i) for name in ENTRIES for i in range(len(BS.CASES[name]))]


@pytest.mark.parametrize("name, i", ROWS, ids=[f"{name}-{BS.CASES[name][i][0]}" for name, i in ROWS])
def test_bounds(name, i):
    G.run(BS.CASES[name][i][1], device="cuda")
