"""gf3_window_frames inside guard bands (tests/guarded.py): dressings A, B and plain, plain and skewed by one element,
bit-for-bit equal outputs and untouched bands.  This only compares bytes.

The rows are entered in the table of tests/test_bounds_signal_gpu.py (`BS.case`), which is the table the census of
tests/test_guarded_cpu.py reads, as tests/test_bounds_stbc_gpu.py enters its own: importing this module is what gives the
entry its rows there, and they run here.  That module's geometry (N = 1024, CP = 32, three packets in every sample
storage, placed at both ends of the samples and ragged beyond them): a ramp of 5 samples and one of the whole prefix, a
stream with a NaN inside a ramp and an Inf inside the prefix stretch that is folded in, and F = 0."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import test_bounds_signal_gpu as BS

pytestmark = pytest.mark.gpu
ENTRIES = ("gf3_window_frames",)
f64, i32 = torch.float64, torch.int32


def ramp(L):
    return 0.5 - 0.5 * np.cos(np.pi * (np.arange(L) + 0.5) / L)


for st in BS.STORAGES:
    for L in (5, BS.CP):
        for planted in ((False, True) if st in ("f64", "f32") and L == 5 else (False,)):
            for empty in ((False, True) if L == BS.CP else (False,)):
                @BS.case("gf3_window_frames", f"{st}-L{L}{'-nonfinite' if planted else ''}{'-F0' if empty else ''}")
                def _(a, st=st, L=L, planted=planted, empty=empty):
                    s = BS.setup(st)
                    p = s.p
                    samples = s.x
                    if planted:                                 # packet 1: symbol 1's ramp, symbol 2's folded stretch
                        samples = s.x.copy()
                        samples[s.starts[1] + 2 * p.S - 2] = np.nan
                        samples[s.starts[1] + 2 * p.S + p.CP - 1] = np.inf
                    x = a.in_("d_in", samples, samples=True)
                    off, ragged = BS.placed(len(s.x), s.L, int(s.starts[1]))
                    off = a.in_("d_offsets", off)
                    rows = len(ragged)
                    F = 0 if empty else rows
                    r = a.in_("d_ramp_f64", ramp(L))
                    out = a.out("d_out", (rows, s.L), BS.TORCH_OF[st])
                    report = a.out("d_report_f64", (rows, p.M, 2), f64)
                    status = a.out("d_status_i32", (rows,), i32)
                    BS.finish(a, s, s.lib.gf3_window_frames(s.h, BS.ptr(x), x.numel(), BS.ptr(off), F, BS.ptr(r), L, BS.ptr(out),
                                                            BS.ptr(report), BS.ptr(status), s.stream()), F)
                    if F:
                        assert status.tolist() == ragged.astype(int).tolist()
                        nan = torch.isnan(report).all(dim=2).cpu().numpy()
                        want = np.repeat(ragged[:, None], p.M, axis=1)
                        if planted:                             # (offsets[6] is packet 1)
                            want[6, 1] = want[6, 2] = True
                        assert np.array_equal(nan, want)


ROWS = [(name, i) for name in ENTRIES for i in range(len(BS.CASES[name]))]


@pytest.mark.parametrize("name, i", ROWS, ids=[f"{name}-{BS.CASES[name][i][0]}" for name, i in ROWS])
def test_bounds(name, i):
    G.run(BS.CASES[name][i][1], device="cuda")
