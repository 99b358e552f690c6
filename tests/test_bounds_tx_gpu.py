"""The transmit-side ABI entries inside guard bands (tests/guarded.py): gf3_tx_frames, gf3_tx_frames_ex and
gf3_tone_reserve.  This only compares bytes; the values are held by tests/test_gpu_parity.py and tests/test_papr_gpu.py.

The rows are entered in the table of tests/test_bounds_signal_gpu.py (`BS.case`) and run here (ENTRIES), on that file's
geometry: N = 1024, comb3 (C = 171, so Ku = 340 reserved carriers), P = 1, D = 3, three packets.
A row of gf3_tx_frames is `stride` samples, all of them promised, zeros included: with `stride` exactly one packet and no
gaps the last sample of the last row lies against the band; with `stride` 13 longer and gaps [0, 13, 6] the second packet
ends on its row's last sample.  A stride one sample short of a packet is refused and nothing is written.  One more
geometry, `wide` of tests/test_bounds_symbols_gpu.py (N = 2048, carriers 1 .. 600: a contiguous map, which the kernels
resolve without the position table, Ku = 423), runs the N = 2048 kernels."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import tables as T
from tests import test_bounds_signal_gpu as BS
from tests import test_bounds_symbols_gpu as SY

pytestmark = pytest.mark.gpu
ENTRIES = ("gf3_tx_frames", "gf3_tx_frames_ex", "gf3_tone_reserve")
c128, f64, f32, u8 = torch.complex128, torch.float64, torch.float32, torch.uint8
F = BS.NF
EINVAL = -1
DT = dict(f64=(0, f64), f32=(1, f32))                              # gf3_dtype, torch type
ptr = BS.ptr


def payload(a, s, seed):
    return a.in_("d_bits_packed", np.random.default_rng(seed).integers(0, 256, (F, s.bpf)).astype(np.uint8))


def packet_len(p):
    return p.Lc + (2 * p.P + p.D) * p.S


# (label, stride beyond one packet, gaps, refused)
LAYOUTS = (("exact", 0, None, False), ("gaps", 13, [0, 13, 6], False), ("short", -1, None, True))
TX_RUNS = [(tb, dt, lay) for tb, dt in (("qpsk_ref", "f64"), ("qpsk_ref", "f32"), ("rect8", "f64")) for lay in LAYOUTS]
TX_RUNS += [("wide", "f32", LAYOUTS[0]), ("wide", "f64", LAYOUTS[1])]
for ex in (False, True):
    k = 0
    for tb, dt, (lay, extra, gaps, refused) in TX_RUNS:
        for empty in ((False, True) if k == 0 else (False,)):
            @BS.case("gf3_tx_frames_ex" if ex else "gf3_tx_frames", f"{tb}-{dt}-{lay}{'-F0' if empty else ''}")
            def _(a, ex=ex, tb=tb, dt=dt, extra=extra, gaps=gaps, refused=refused, empty=empty):
                s = SY.setup("wide") if tb == "wide" else BS.setup("f64", tb)
                p, rng = s.p, np.random.default_rng(2)
                bits = payload(a, s, 1)
                stride = packet_len(p) + extra
                d_gaps = a.in_("d_gaps", np.array(gaps, dtype=np.int64)) if gaps else None
                out = a.out("d_out", (F, stride), DT[dt][1])
                n = 0 if empty else F
                if ex:                                          # tones instead of the filler ("which may then be NULL"), half gain
                    tones = a.in_("d_tones_c128", 0.3 * (rng.normal(size=(F, p.D, p.K - p.C)) + 1j * rng.normal(size=(F, p.D, p.K - p.C))))
                    rc = s.lib.gf3_tx_frames_ex(s.h, ptr(bits), None, ptr(d_gaps), n, ptr(out), stride, DT[dt][0], ptr(tones), 0.5,
                                                s.stream())
                else:
                    fill = a.in_("d_filler_c128", T.QPSK_FILL[rng.integers(0, 4, p.K)])
                    rc = s.lib.gf3_tx_frames(s.h, ptr(bits), ptr(fill), ptr(d_gaps), n, ptr(out), stride, DT[dt][0], s.stream())
                BS.finish(a, s, rc, n, want=EINVAL if refused and n else 0)
                if n and gaps:                                  # the zeros in front of a packet and behind it are written
                    assert not out[1, :13].any() and out[1, -1] != 0 and not out[2, :6].any() and not out[2, -7:].any()
        k += 1


for geom, iterations, empty in (("base", 0, False), ("base", 0, True), ("base", 3, False), ("base", 65, False), ("wide", 3, False)):
    @BS.case("gf3_tone_reserve", f"{geom}-iter{iterations}{'-refused' if iterations > 64 else ''}{'-F0' if empty else ''}")
    def _(a, geom=geom, iterations=iterations, empty=empty):
        s = SY.setup("wide") if geom == "wide" else BS.setup("f64", "qpsk_ref")
        p = s.p
        bits = payload(a, s, 3)
        tones = a.out("d_tones_c128", (F, p.D, p.K - p.C), c128)
        report = a.out("d_report_f64", (F, p.D, 4), f64)
        n = 0 if empty else F
        rc = s.lib.gf3_tone_reserve(s.h, ptr(bits), n, 4.0, 6.0, iterations, ptr(tones), ptr(report), s.stream())
        BS.finish(a, s, rc, n, want=EINVAL if iterations > 64 else 0)


ROWS = [(name, i) for name in ENTRIES for i in range(len(BS.CASES[name]))]


@pytest.mark.parametrize("name, i", ROWS, ids=[f"{name}-{BS.CASES[name][i][0]}" for name, i in ROWS])
def test_bounds(name, i):
    G.run(BS.CASES[name][i][1], device="cuda")
