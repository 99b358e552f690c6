"""The three sample readers that are not packet-placed inside guard bands (tests/guarded.py): gf3_schmidl_cox,
gf3_resample_stream and gf3_debug_demod_screen.  This only compares bytes; the values are held by tests/test_gpu_parity.py,
tests/test_rate_gpu.py and tests/test_demod_screen_gpu.py.

The rows are entered in the table of tests/test_bounds_signal_gpu.py (`BS.case`) and run here (ENTRIES), on that file's
streams in every sample storage; next to an integer sample array the bands hold the type's extremes.
    gf3_schmidl_cox         n = search_len - 1 + 2L exactly: tap d + 2L of the last lag is the array's last sample.
                            search_len 2 (one lag), 4097 (exactly one 4096-lag chunk) and 4101 (the carry and a partial chunk of 4).
    gf3_resample_stream     1025 outputs (two tiles of 512 and one output) at five ratios, as a whole stream whose last
                            outputs' taps run past the buffer's end, and as a block at in_origin = 700 whose first outputs
                            reach in front of the buffer and whose last tap is the buffer's last sample.
    gf3_debug_demod_screen  the placements of `BS.frames_in`; a ragged packet keeps its rows of d_ep32 and d_E."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import test_bounds_signal_gpu as BS

pytestmark = pytest.mark.gpu
ENTRIES = ("gf3_schmidl_cox", "gf3_resample_stream", "gf3_debug_demod_screen")
c64, f32, i64, i32, u8 = torch.complex64, torch.float32, torch.int64, torch.int32, torch.uint8
EINVAL = -1
ptr = BS.ptr

for st in BS.STORAGES:
    # (4097 in one storage: exactly one chunk of 4096 lags)
    for search_len, short in ((2, False), (4101, False), (4101, True)) + (((4097, False),) if st == "f64" else ()):
        @BS.case("gf3_schmidl_cox", f"{st}-S{search_len}{'-short' if short else ''}")
        def _(a, st=st, search_len=search_len, short=short):
            s = BS.setup(st)
            n = search_len - 1 + 2 * (s.p.K + 1) - (1 if short else 0)    # "Needs n >= search_len - 1 + 2L samples"
            x = a.in_("d_r", s.full[:n], samples=True)
            index = a.out("d_index", (1,), i64)
            BS.finish(a, s, s.lib.gf3_schmidl_cox(s.h, ptr(x), n, search_len, ptr(index), s.stream()), want=EINVAL if short else 0)


# ---- gf3_resample_stream -----------------------------------------------------------------------------------------------------------
RATIOS = ((1.0, 16), (44100 / 48000, 32), (48000 / 44100, 16), (4.0, 32), (0.25, 16))
N_OUT = 1025


def stream_plan(r, T, block):
    """(in_origin, j0, n_in).  whole: the buffer ends on the sample the last output reads at, so the taps behind it run past
    the end (and those of the first outputs lie in front of sample 0).  block: the buffer starts at sample 700, j0 is three
    outputs before the first whose taps all lie inside, and the buffer's last sample is the last output's last tap."""
    Tw = int(np.ceil(T * r)) if r > 1 else T
    at = lambda j: int(np.floor(float(j) * r))
    if not block:
        return 0, 0, at(N_OUT - 1) + 1
    j = 0
    while at(j) - Tw + 1 < 700:
        j += 1
    j0 = j - 3
    assert at(j0) - Tw + 1 < 700 <= at(j) - Tw + 1
    return 700, j0, at(j0 + N_OUT - 1) + Tw - 700 + 1


def samples_of(storage, n, seed):
    rng = np.random.default_rng(seed)
    if storage == "u8":
        return rng.integers(0, 256, n).astype(np.uint8)
    if storage == "i16":
        return rng.integers(-20000, 20001, n).astype(np.int16)
    return (3000.0 * rng.normal(size=n)).astype(np.float64 if storage == "f64" else np.float32)


k = 0
for r, T in RATIOS:
    for ctx in ("f32", "i16"):
        for block in (False, True):
            in_st = BS.STORAGES[k % 4]
            k += 1

            @BS.case("gf3_resample_stream", f"r{r:.4f}-T{T}-{in_st}-to-{ctx}-{'block' if block else 'whole'}")
            def _(a, r=r, T=T, ctx=ctx, block=block, in_st=in_st):
                s = BS.setup(ctx)
                origin, j0, n_in = stream_plan(r, T, block)
                x = a.in_("d_in", samples_of(in_st, n_in, T), samples=True)
                out = a.out("d_out", (N_OUT,), BS.TORCH_OF[ctx])
                BS.finish(a, s, s.lib.gf3_resample_stream(s.h, ptr(x), BS.STORAGES.index(in_st), n_in, origin, r, T, j0, N_OUT, ptr(out),
                                                          s.stream()))


@BS.case("gf3_resample_stream", "no-outputs-no-addresses")
def _(a):                                                           # "n_out == 0 is a no-op and needs no addresses"
    s = BS.setup("f32")
    BS.finish(a, s, s.lib.gf3_resample_stream(s.h, None, 2, 0, 0, 1.0, 16, 0, 0, None, s.stream()))


# ---- gf3_debug_demod_screen --------------------------------------------------------------------------------------------------------
for st in BS.NARROW:
    for empty in ((False, True) if st == BS.NARROW[0] else (False,)):
        @BS.case("gf3_debug_demod_screen", f"{st}-qpsk_ref{'-F0' if empty else ''}")
        def _(a, st=st, empty=empty):
            s = BS.setup(st, "qpsk_ref")
            p = s.p
            x, off, F, rows, ragged = BS.frames_in(a, s, empty)
            bits = a.out("d_bits_packed", (rows, s.bpf), u8)
            ep32, E = a.out("d_ep32", (rows, p.D, p.C), c64), a.out("d_E", (rows, p.D), f32)
            cls = a.out("d_cls", (rows,), i32)
            # [count | pad to 64 bytes | listed packet numbers]: the count word is promised, the pad and the order of the
            # entries behind it are not
            work = a.out("d_list", (s.lib.gf3_demod_screen_workspace_bytes(s.h, rows),), u8, align=G.WORK_ALIGN)
            a.unspecified("d_list", np.s_[4:])
            BS.finish(a, s, s.lib.gf3_debug_demod_screen(s.h, ptr(x), x.numel(), ptr(off), F, ptr(bits), ptr(ep32), ptr(E), ptr(cls),
                                                         ptr(work), s.stream()), F)
            if F:                                               # a ragged packet: a zero row of bits, verdict 0, its rows of
                a.keep("d_ep32", ragged)                        # d_ep32 and d_E not written
                a.keep("d_E", ragged)
                bad = torch.from_numpy(ragged).to(bits.device)
                assert not bits[bad].any() and not cls[bad].any() and int(work[:4].view(torch.int32).item()) == int(cls.sum())


ROWS = [(name, i) for name in ENTRIES for i in range(len(BS.CASES[name]))]


@pytest.mark.parametrize("name, i", ROWS, ids=[f"{name}-{BS.CASES[name][i][0]}" for name, i in ROWS])
def test_bounds(name, i):
    G.run(BS.CASES[name][i][1], device="cuda")
