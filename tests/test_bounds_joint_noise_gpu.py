"""The ABI entries of the two-speaker paths under coloured noise inside guard bands (tests/guarded.py): dressings A, B and
plain, plain and skewed by one element, bit-for-bit equal outputs and untouched bands.  This only compares bytes.

The rows are entered in the table of tests/test_bounds_signal_gpu.py (`BS.case`), which is the table the census of
tests/test_guarded_cpu.py reads, as tests/test_bounds_mimo_gpu.py and tests/test_bounds_stbc_gpu.py enter theirs: importing
this module is what gives the four entries their rows there, and they run here.  The geometry is that module's with P = 4
(the estimate needs pilot symbols beyond the two the covers take) and D = 2 (the space-time code pairs the data symbols):
N = 1024, CP = 32, the carrier map comb3 (C = 171: one partial 256-carrier tile), two packets; the estimate reads the samples
in every storage at that module's placements (first sample, last sample, ragged at either end)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import guarded as G
from tests import tables as T
from tests import test_bounds_signal_gpu as BS

pytestmark = pytest.mark.gpu
ENTRIES = ("gf3_mimo_pilot_noise", "gf3_joint_noise_weights", "gf3_mimo_detect_nw", "gf3_stbc_detect_nw")
c128, f64, f32, i32 = torch.complex128, torch.float64, torch.float32, torch.int32
P, D, NF = 4, 2, 2


@functools.lru_cache(maxsize=None)
def setup(storage="f64"):
    """BS.setup's stream and cut with this module's P, D and two packets"""
    from gf3_audio_modem_amd import _lib
    from tests.util import engine_for
    s = BS.Setup()
    p = T.params_for("qpsk_ref", BS.N, T.comb3(BS.N // 2 - 1), P=P, D=D, CP=BS.CP)
    rs = np.random.RandomState(7)
    payload = T.existing_labels_payload(rs, p, NF * D * p.C)
    gaps = np.array([0, 11])
    r = orc.tx_stream(payload, rs.choice(T.QPSK_FILL, size=p.K - p.C), p, gaps=gaps, lead=0, tail=2)
    r = r + 0.01 * np.sqrt(np.mean(r * r)) * rs.randn(len(r))
    full = BS.quantised(r, storage)
    body = np.cumsum(gaps) + np.arange(NF) * p.frame_len + p.Lc
    s.L = p.M * p.S
    s.x = full[body[0]: body[-1] + s.L].copy()
    s.starts = (body - body[0]).astype(np.int64)
    s.p, s.eng = p, engine_for(p, in_dtype=BS.TORCH_OF[storage])
    s.lib, s.h, s.stream, s.err = s.eng.lib, s.eng._h, s.eng._stream, _lib.last_error
    assert p.C % 256
    return s


for st in BS.STORAGES:
    for empty in ((False, True) if st == "f64" else (False,)):
        @BS.case("gf3_mimo_pilot_noise", f"{st}{'-F0' if empty else ''}")
        def _(a, st=st, empty=empty):
            s = setup(st)
            x, off, F, rows, ragged = BS.frames_in(a, s, empty)
            rng = np.random.default_rng(1)
            H = a.in_("d_H_c128", rng.normal(size=(rows, 2, 2, s.p.K)) + 1j * rng.normal(size=(rows, 2, 2, s.p.K)))
            var = a.out("d_var_out_f64", (rows, 2, s.p.K), f64)
            status = a.out("d_status_i32", (rows,), i32)
            BS.finish(a, s, s.lib.gf3_mimo_pilot_noise(s.h, BS.ptr(x), x.numel(), BS.ptr(off), F, BS.ptr(H), BS.ptr(var), BS.ptr(status),
                                                       s.stream()), F)
            if F:                                               # a ragged packet: status 1 and NaN rows, written
                assert status.tolist() == ragged.astype(int).tolist()
                bad = torch.from_numpy(ragged).to(var.device)
                assert torch.isnan(var[bad]).all() and torch.isfinite(var[~bad]).all()


def branches(a, s, B, F, planted, spectra=True):
    """B branches of seeded estimates, slopes (and spectra) as `in_` arrays, the weights [B, F, C] -> the pointer tables, the
    one slope array of the space-time code, the weights"""
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
    w = np.exp(rng.normal(size=(B, F, p.C)))
    if planted:
        w[0, 0, 7], w[:, F - 1, 9], w[B - 1, 0, 11] = 0.0, 0.0, np.nan
    tab = lambda xs: (C.c_void_p * B)(*[x.data_ptr() for x in xs])
    return tab(Ys), tab(Hs), tab(Ss), Ss[0], a.in_("d_w_f64", w)


for B in (1, 2, 3, 4):
    for planted in ((False, True) if B == 2 else (False,)):
        for empty in ((False, True) if B == 2 and not planted else (False,)):
            label = f"B{B}{'-nonfinite' if planted else ''}{'-F0' if empty else ''}"

            @BS.case("gf3_joint_noise_weights", label)
            def _(a, B=B, planted=planted, empty=empty):
                s = setup()
                p = s.p
                rng = np.random.default_rng(10 + B)
                vs = []
                for b in range(B):
                    v = rng.chisquare(4, size=(NF, 2, p.K))
                    if planted:                                 # a NaN in one branch of packet 0; packet 1 all zero: weights 1
                        v[0, 1, p.data_carriers[3] - 1] = np.nan if b == 0 else 1.0
                        v[1] = 0.0
                    vs.append(a.in_(f"d_var_f64[{b}]", v))
                w = a.out("d_w_out_f64", (B, NF, p.C), f64)
                F = 0 if empty else NF
                tab = (C.c_void_p * B)(*[v.data_ptr() for v in vs])
                BS.finish(a, s, s.lib.gf3_joint_noise_weights(s.h, B, tab, F, BS.ptr(w), s.stream()), F)
                if F:
                    assert torch.isfinite(w).all()

            @BS.case("gf3_mimo_detect_nw", label)
            def _(a, B=B, planted=planted, empty=empty):
                s = setup()
                p = s.p
                Yt, Ht, St, _, w = branches(a, s, B, NF, planted)
                llr = a.out("d_llr_f32", (NF, 2, p.D, p.C, p.mu), f32)
                F = 0 if empty else NF
                BS.finish(a, s, s.lib.gf3_mimo_detect_nw(s.h, B, Yt, Ht, St, BS.ptr(w), F, BS.ptr(llr), s.stream()), F)
                if F:
                    assert torch.isfinite(llr).all()

            @BS.case("gf3_stbc_detect_nw", label)
            def _(a, B=B, planted=planted, empty=empty):
                s = setup()
                p = s.p
                Yt, Ht, _, slope, w = branches(a, s, B, NF, planted)
                llr = a.out("d_llr_f32", (NF, p.D, p.C, p.mu), f32)
                F = 0 if empty else NF
                BS.finish(a, s, s.lib.gf3_stbc_detect_nw(s.h, B, Yt, Ht, BS.ptr(slope), BS.ptr(w), F, BS.ptr(llr), s.stream()), F)
                if F:
                    assert torch.isfinite(llr).all()


ROWS = [(name, i) for name in ENTRIES for i in range(len(BS.CASES[name]))]


@pytest.mark.parametrize("name, i", ROWS, ids=[f"{name}-{BS.CASES[name][i][0]}" for name, i in ROWS])
def test_bounds(name, i):
    G.run(BS.CASES[name][i][1], device="cuda")
