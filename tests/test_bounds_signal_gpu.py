"""Every signal-path ABI entry inside guard bands (tests/guarded.py): no byte outside the arrays the header gives a call is
read into a result or written, every promised element is written, every documented not-written range keeps its pre-fill.

One table row (a key of CASES) per entry that reads samples through (d_in, n_in, offsets) or (d_in, n_in, stride, window);
the coding entries are in tests/test_bounds_coding_gpu.py, and tests/test_guarded_cpu.py holds the two tables, its EXEMPT
list and its WITHHELD list (the entries still owed a row, with the reason) to cover `_lib._SIGS`.  Sibling files enter
their rows in THIS table through `case` and run them themselves (their ENTRIES): test_bounds_mimo_gpu.py,
test_bounds_mimo_known_gpu.py, test_bounds_stbc_gpu.py and test_bounds_joint_noise_gpu.py (the two-speaker entries),
test_bounds_symbols_gpu.py (everything that takes equalised symbols, spectra or bits), test_bounds_tx_gpu.py (the transmit
side) and test_bounds_samples_gpu.py (gf3_schmidl_cox, gf3_resample_stream, gf3_debug_demod_screen).  Calls go through
`eng.lib.<name>(eng._h, ...)`, the explicit-workspace forms wherever they exist.

Geometry: N = 1024, CP = 32, P = 1 (2 where the denoiser needs pilot repeats), D = 3 (odd: the symbol-pair kernels end on a
single symbol), the carrier map comb3 (C = 171, odd, not contiguous), QPSK (C mu = 342) and the 3-bit rect8 (C mu = 513:
rows end inside a byte), three packets, every sample storage for the entries that read samples.
Placements of every (d_in, n_in, offsets) entry: the first item starts at sample 0, the last ends at sample n_in - 1 with
the band right behind it, and between them items ragged at either end (-1, n_in - len + 1, n_in, +-2^40); F = 0 writes
nothing.  The frames sync runs with its first window starting at sample 0 and its last lag ending on the last sample, and
with windows that start in front of the array and run past its end.
Not-written ranges the cases name: the dump rows (eq, Hs, He, slope, Hest) of a ragged packet; the output row of the absent
second half of an odd pair transform; d_starts of a window the frames screen leaves unresolved."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import guarded as G
from tests import tables as T

pytestmark = pytest.mark.gpu
TORCH_OF = dict(f64=torch.float64, f32=torch.float32, i16=torch.int16, u8=torch.uint8)
STORAGES = ("f64", "f32", "i16", "u8")
NARROW = ("f32", "i16", "u8")                                       # what the fp32 screens of the demodulator take
DEMOD_RUNS = [(st, "qpsk_ref") for st in STORAGES] + [("f64", "rect8")]
c128, c64, f64, f32, i64, i32, u8 = (torch.complex128, torch.complex64, torch.float64, torch.float32, torch.int64, torch.int32,
                                     torch.uint8)
N, CP, D, NF = 1024, 32, 3, 3
CASES = {}


def case(entry, label):
    def register(fn):
        CASES.setdefault(entry, []).append((label, fn))
        return fn
    return register


class Setup:
    pass


def quantised(r, storage):
    if storage == "u8":
        return np.clip(np.rint(128 + 100 * r / np.abs(r).max()), 0, 255).astype(np.uint8)
    return T.quantise(r, dict(f64="float64", f32="float32", i16="int16")[storage])


@functools.lru_cache(maxsize=None)
def setup(storage="f64", table="qpsk_ref", P=1):
    """Engine, the stream of three packets with its terminating chirp (`full`), and the cut `x` of it whose first sample is
    the first packet body's first and whose last sample is the last body's last; `starts` are the bodies in `x`."""
    from gf3_audio_modem_amd import _lib
    from tests.util import engine_for
    s = Setup()
    p = T.params_for(table, N, T.comb3(N // 2 - 1), P=P, D=D, CP=CP)
    rs = np.random.RandomState(7)
    payload = T.existing_labels_payload(rs, p, NF * D * p.C)
    fill = rs.choice(T.QPSK_FILL, size=p.K - p.C)
    gaps = np.array([0, 11, 6])
    r = orc.tx_stream(payload, fill, p, gaps=gaps, lead=0, tail=2)
    r = r + 0.01 * np.sqrt(np.mean(r * r)) * rs.randn(len(r))
    s.full = quantised(r, storage)
    body = np.cumsum(gaps) + np.arange(NF) * p.frame_len + p.Lc
    s.L = p.M * p.S
    s.x = s.full[body[0]: body[-1] + s.L].copy()
    s.starts = (body - body[0]).astype(np.int64)
    s.p, s.storage, s.tb, s.eng = p, storage, table, engine_for(p, in_dtype=TORCH_OF[storage])
    s.lib, s.h, s.stream, s.bpf, s.err = s.eng.lib, s.eng._h, s.eng._stream, s.eng.bytes_per_frame, _lib.last_error
    assert p.C % 2 == 1 and (p.C * p.mu) % 8
    return s


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def finish(a, s, rc, F=1, want=0):
    a.result("rc", rc)
    assert rc == want, (rc, s.err())
    if F == 0 or rc != 0:
        a.keep_all()


def placed(n, L, inside):
    """Offsets of items of L samples in n: first at 0, ragged at either end, one in the middle, last ending at n.
    -> (offsets int64 [8], ragged bool [8])"""
    off = np.array([0, -1, n - L + 1, n, 2 ** 40, -2 ** 40, inside, n - L], dtype=np.int64)
    return off, np.array([0, 1, 1, 1, 1, 1, 0, 0], dtype=bool)


def frames_in(a, s, empty=False, L=None):
    """d_in, d_offsets, the F to pass, the number of rows to allocate, which of them are ragged."""
    x = a.in_("d_in", s.x, samples=True)
    off, ragged = placed(len(s.x), s.L if L is None else L, int(s.starts[1]))
    return x, a.in_("d_offsets", off), (0 if empty else len(off)), len(off), ragged


def dumps(a, s, rows, ragged, names):
    """The optional demodulator outputs `names` (the others None).  A ragged packet's rows are not written."""
    p = s.p
    kinds = dict(eq=((rows * p.D, p.C), c128), Hs=((rows, p.K), c128), He=((rows, p.K), c128), slope=((rows,), f64),
                 Hest=((rows, p.D, p.K), c128))
    o = {}
    for k, (shape, dt) in kinds.items():
        o[k] = a.out("d_" + k, shape, dt) if k in names else None
        if k in names:
            a.keep("d_" + k, np.repeat(ragged, p.D) if k == "eq" else ragged)
    return o


ALL_DUMPS = ("eq", "Hs", "He", "slope", "Hest")


def demod(a, entry, st, tb, names=(), empty=False, P=1, mode=1, precision=-1, work=False, threshold=9.0, report=True,
          weight=None):
    """One call of the demodulator family."""
    s = setup(st, tb, P)
    p, lib = s.p, s.lib
    x, off, F, rows, ragged = frames_in(a, s, empty)
    o = dumps(a, s, rows, ragged, names)
    status = a.inout("d_status", np.zeros(1, np.int32))
    d_work = a.work("d_work", lib.gf3_demod_workspace_bytes(s.h, F)) if work else None
    head = (s.h, ptr(x), x.numel(), ptr(off), F)
    if entry == "gf3_demod_frames_llr":
        llr = a.out("d_llr_f32", (rows * p.D * p.C * p.mu,), f32)
        rc = lib.gf3_demod_frames_llr(*head, ptr(llr), weight, ptr(o["Hs"]), ptr(o["He"]), ptr(o["slope"]), ptr(status),
                                      ptr(d_work), mode, s.stream())
        if F:
            assert not llr.reshape(rows, -1)[torch.from_numpy(ragged).to(llr.device)].view(torch.int32).any()      # rows of +0.0f
        return finish(a, s, rc, F)
    bits = a.out("d_bits_packed", (rows, s.bpf), u8)
    outs = (ptr(bits), ptr(o["eq"]), ptr(o["Hs"]), ptr(o["He"]), ptr(o["slope"]), ptr(o["Hest"]), ptr(status))
    if entry == "gf3_demod_frames":
        rc = lib.gf3_demod_frames(*head, *outs, s.stream())
    elif entry == "gf3_demod_frames_ex":
        rc = lib.gf3_demod_frames_ex(*head, *outs, ptr(d_work), mode, s.stream())
    elif entry == "gf3_demod_frames_px":
        rc = lib.gf3_demod_frames_px(*head, *outs, ptr(d_work), mode, precision, s.stream())
    else:
        rep = a.out("d_report", (rows, 2, 5), f64) if report else None
        rc = lib.gf3_demod_frames_dn(*head, *outs, ptr(d_work), threshold, ptr(rep), s.stream())
    finish(a, s, rc, F)
    if F:
        torch.cuda.synchronize()
        assert int(status.item()) == 1 and not bits[torch.from_numpy(ragged).to(bits.device)].any()    # ragged: zero bits, bit 0 set


def demod_cases(entry, runs, variants):
    for st, tb in runs:
        for label, kw in variants:
            for empty in ((False, True) if (st, tb) == runs[0] else (False,)):
                @case(entry, f"{st}-{tb}-{label}{'-F0' if empty else ''}")
                def _(a, st=st, tb=tb, kw=kw, empty=empty):
                    demod(a, entry, st, tb, empty=empty, **kw)


demod_cases("gf3_demod_frames", DEMOD_RUNS, [("bits", {}), ("dumps", dict(names=ALL_DUMPS))])
demod_cases("gf3_demod_frames_ex", DEMOD_RUNS, [
    ("one-bits", dict(mode=1, work=True)), ("one-dumps", dict(mode=1, work=True, names=ALL_DUMPS)),
    ("two-bits", dict(mode=2, work=True)), ("two-dumps", dict(mode=2, work=True, names=ALL_DUMPS)),
    ("auto-nowork", dict(mode=0))])
demod_cases("gf3_demod_frames_px", [(st, "qpsk_ref") for st in NARROW], [
    ("screened-bits", dict(precision=1)), ("screened-estimates", dict(precision=1, names=("Hs", "He", "slope"))),
    ("fp64-bits", dict(precision=0))])
demod_cases("gf3_demod_frames_dn", DEMOD_RUNS, [
    ("bits", dict(P=2, work=True, report=False)), ("dumps-report", dict(P=2, work=True, names=ALL_DUMPS))])
demod_cases("gf3_demod_frames_llr", DEMOD_RUNS + [("f32", "rect8")], [
    (f"{wn}-{fn}", dict(weight=w, **kw, names=names))
    for w, wn in ((0, "unit"), (1, "csi"))
    for fn, kw, names in (("fused", dict(mode=1), ()), ("split", dict(mode=2, work=True), ("Hs", "He", "slope")))])


for st in STORAGES:
    for empty in ((False, True) if st == "f64" else (False,)):
        for report in (True, False):
            @case("gf3_denoise_pilots", f"{st}-{'report' if report else 'noreport'}{'-F0' if empty else ''}")
            def _(a, st=st, empty=empty, report=report):
                s = setup(st, "qpsk_ref", 2)
                x, off, F, rows, ragged = frames_in(a, s, empty)
                psum = a.out("d_psum_out", (rows, 2, N), f64)
                rep = a.out("d_report", (rows, 2, 5), f64) if report else None
                finish(a, s, s.lib.gf3_denoise_pilots(s.h, ptr(x), x.numel(), ptr(off), F, 9.0, ptr(psum), ptr(rep), s.stream()), F)

        for entry, dt in (("gf3_rfft_batch", c128), ("gf3_debug_rfft_sp_batch", c64), ("gf3_debug_rfft_sp_pair_batch", c64)):
            if dt == c64 and st == "f64":
                continue
            for odd in ((False, True) if entry.endswith("pair_batch") else (False,)):
                @case(entry, f"{st}{'-odd' if odd else ''}{'-F0' if empty else ''}")
                def _(a, st=st, empty=empty, entry=entry, dt=dt, odd=odd):
                    s = setup(st)
                    x, off, n_sym, rows, _ = frames_in(a, s, empty, L=N)
                    n_sym = n_sym - 1 if odd and n_sym else n_sym        # the last pair has no second half: its row stays
                    out = a.out("d_out", (rows, N // 2 + 1), dt)
                    a.keep("d_out", np.s_[n_sym:])
                    finish(a, s, getattr(s.lib, entry)(s.h, ptr(x), x.numel(), ptr(off), n_sym, ptr(out), s.stream()), n_sym)

        @case("gf3_equalise_known_h", f"{st}{'-F0' if empty else ''}")
        def _(a, st=st, empty=empty):
            s = setup(st)
            p = s.p
            x, off, n_sym, rows, _ = frames_in(a, s, empty, L=N)
            taps = a.in_("d_h", np.array([1.0, 0.4, -0.2, 0.1, 0.05]))
            eq = a.out("d_eq_c128", (rows, p.C), c128)
            bits = a.out("d_bits_u8", (rows * p.C * p.mu,), u8)
            idx = a.out("d_idx_u8", (rows, p.C), u8) if st != "f32" else None
            work = a.work("d_work", s.lib.gf3_known_h_workspace_bytes(s.h, n_sym))
            finish(a, s, s.lib.gf3_equalise_known_h(s.h, ptr(x), x.numel(), ptr(off), n_sym, ptr(taps), 5, ptr(eq), ptr(bits),
                                                    ptr(idx), ptr(work), s.stream()), n_sym)

        @case("gf3_blank_impulses", f"{st}{'-F0' if empty else ''}")
        def _(a, st=st, empty=empty):
            s = setup(st)
            M = s.p.M
            x, off, F, rows, ragged = frames_in(a, s, empty)
            out = a.inout("d_out", s.x, samples=True)
            energy, level = a.out("d_energy_f64", (rows, M), f64), a.out("d_level_f64", (rows, 2), f64)
            counts = a.out("d_counts_i32", (rows, M), i32)
            finish(a, s, s.lib.gf3_blank_impulses(s.h, ptr(x), x.numel(), ptr(off), F, 2.5, 8, ptr(out), ptr(energy), ptr(level),
                                                  ptr(counts), s.stream()), F)
            if F:
                assert (counts[torch.from_numpy(ragged).to(counts.device)] == -1).all() and (counts[0] >= 0).all()

        for taps in (16, 32):
            @case("gf3_resample_frames", f"{st}-T{taps}{'-F0' if empty else ''}")
            def _(a, st=st, empty=empty, taps=taps):
                s = setup(st)
                x, off, F, rows, ragged = frames_in(a, s, empty)
                eps = a.in_("d_eps_f64", np.array([1e-4, 0.0, 0.0, 0.0, 0.0, 0.0, float("nan"), -1e-4]))
                out = a.out("d_out", (rows, s.L), TORCH_OF[st])
                status = a.out("d_status_i32", (rows,), i32)
                finish(a, s, s.lib.gf3_resample_frames(s.h, ptr(x), x.numel(), ptr(off), F, ptr(eps), taps, ptr(out), ptr(status),
                                                       s.stream()), F)
                if F:
                    assert status.tolist() == [0, 1, 1, 1, 1, 1, 2, 0]


# ---- frames sync: window f is [f stride + win_lo, f stride + win_hi) ----------------------------------------------------------
def windows(s, how):
    """(samples, stride, win_lo, win_hi): `exact` -- the first window starts at sample 0 and the last lag of the last
    window takes the array's last sample; `ragged` -- the first window starts before the array and the last one's taps run
    past its end."""
    stride, Lc = s.p.frame_len, s.p.Lc
    if how == "exact":
        return s.full[: 2 * stride + 64 + Lc - 1], stride, 0, 64
    return s.full[: 2 * stride + 40 + Lc // 2], stride, -3, 61


for st in STORAGES:
    for how in ("exact", "ragged"):
        for peak in (False, True):
            @case("gf3_sync_frames", f"{st}-{how}{'-peak' if peak else ''}")
            def _(a, st=st, how=how, peak=peak):
                s = setup(st)
                xs, stride, lo, hi = windows(s, how)
                x = a.in_("d_in", xs, samples=True)
                starts = a.out("d_starts", (NF,), i64)
                pk = a.out("d_peak", (NF,), f64) if peak else None
                finish(a, s, s.lib.gf3_sync_frames(s.h, ptr(x), x.numel(), NF, stride, lo, hi, ptr(starts), ptr(pk), s.stream()))

            for mode in (0, 1):
                @case("gf3_sync_frames_ex", f"{st}-{how}-mode{mode}{'-peak' if peak else ''}")
                def _(a, st=st, how=how, peak=peak, mode=mode):
                    s = setup(st)
                    xs, stride, lo, hi = windows(s, how)
                    x = a.in_("d_in", xs, samples=True)
                    starts = a.out("d_starts", (NF,), i64)
                    pk = a.out("d_peak", (NF,), f64) if peak else None
                    work = None
                    if mode == 1:
                        # [count | pad to 64 bytes | list]: the header promises the count word and nothing of the pad or of
                        # the list's entries behind the count, so only the word is compared; the bands hold all of it in
                        work = a.out("d_work", (s.lib.gf3_sync_frames_workspace_bytes(s.h, NF),), u8, align=G.WORK_ALIGN)
                        a.unspecified("d_work", np.s_[4:])
                    finish(a, s, s.lib.gf3_sync_frames_ex(s.h, ptr(x), x.numel(), NF, stride, lo, hi, ptr(starts), ptr(pk), mode,
                                                          ptr(work), s.stream()))
                    if mode == 1 and peak:                          # the all-fp64 fallback: "0 when the call ran all fp64"
                        assert not work[:4].any()

        if st in ("f64", "f32"):
            @case("gf3_sync_frames_ex", f"{st}-{how}-mode1-nowork")
            def _(a, st=st, how=how):                                # "NULL selects mode 0"
                s = setup(st)
                xs, stride, lo, hi = windows(s, how)
                x = a.in_("d_in", xs, samples=True)
                starts = a.out("d_starts", (NF,), i64)
                finish(a, s, s.lib.gf3_sync_frames_ex(s.h, ptr(x), x.numel(), NF, stride, lo, hi, ptr(starts), None, 1, None, s.stream()))

        @case("gf3_debug_frames_screen", f"{st}-{how}")
        def _(a, st=st, how=how):
            s = setup(st)
            xs, stride, lo, hi = windows(s, how)
            x = a.in_("d_in", xs, samples=True)
            starts, y32 = a.out("d_starts", (NF,), i64), a.out("d_y32", (NF, hi - lo), f32)
            err, cls = a.out("d_err", (NF,), f32), a.out("d_cls", (NF,), i32)
            work = a.out("d_work", (s.lib.gf3_sync_frames_workspace_bytes(s.h, NF),), u8, align=G.WORK_ALIGN)
            a.unspecified("d_work", np.s_[4:])
            finish(a, s, s.lib.gf3_debug_frames_screen(s.h, ptr(x), x.numel(), NF, stride, lo, hi, ptr(starts), ptr(y32), ptr(err),
                                                       ptr(cls), ptr(work), s.stream()))
            a.keep("d_starts", (cls == 2).cpu().numpy())             # "d_starts[f] is then left alone"


ROWS = [(name, i) for name in CASES for i in range(len(CASES[name]))]


@pytest.mark.parametrize("name, i", ROWS, ids=[f"{name}-{CASES[name][i][0]}" for name, i in ROWS])
def test_bounds(name, i):
    G.run(CASES[name][i][1], device="cuda")
