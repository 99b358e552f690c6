"""The default frames sync (gf3_sync_frames == gf3_sync_frames_ex mode -1, Engine.sync_frames(screened=None)): the library
takes the fp32 screen with a proven bound in a workspace of its own and the fp64 kernel on the windows the bound leaves
open.  Every check compares with mode 0 (screened=False: the all-fp64 kernel on every window), element for element."""
import functools
import threading

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests.util import engine_for, load, params_of

pytestmark = pytest.mark.gpu

GEOMETRIES = [(1024, 128, 2), (4096, 512, 2), (2048, 256, 6), (4096, 224, 2), (8192, 1024, 2)]   # of test_screened_sync_frames_equals_fp64_and_bound_holds
SCREENED, FP64 = 0, 2                                                                              # gf3_sync_frames_last paths


def _params(N, CP, mu):
    pts, bt = orc.qpsk_table() if mu == 2 else orc.square_qam_table(mu)
    K = N // 2 - 1
    known = load("g6_realrec")["known_bits"]
    known = np.tile(known, -(-K * mu // len(known)))
    return orc.RxParams(N=N, CP=CP, P=2, D=2, lo=1, hi=K, const_points=pts, const_bits=bt, known_bits=known,
                        fit_lo=min(500, K // 2), fit_hi=min(1000, K))


@functools.lru_cache(maxsize=None)
def _rows(N, CP, mu, F=10, gmax=300):
    """F packets with jitter gaps, one per row (fp64, host)."""
    p = _params(N, CP, mu)
    rs = np.random.RandomState(7 * N + mu)
    payload = rs.randint(0, 2, F * p.D * p.C * p.mu)
    fill = np.array([(1 + 1j) / np.sqrt(2)] * (p.K - p.C))
    frames = orc.tx_frames(payload, fill, p)
    gaps = rs.randint(0, gmax, F)
    rows = np.zeros((F, gmax + p.frame_len + 64))
    for f in range(F):
        rows[f, gaps[f]: gaps[f] + p.frame_len] = frames[f]
    return rows


def _store(rows, dt):
    if dt == torch.int16:
        return torch.from_numpy(np.round(np.nan_to_num(rows) * (20000.0 / np.nanmax(np.abs(rows)))).astype(np.int16)).cuda()
    return torch.from_numpy(rows.astype(np.float32) if dt == torch.float32 else rows).cuda()


@pytest.mark.parametrize("dt", [torch.float32, torch.float64, torch.int16], ids=["f32", "f64", "i16"])
@pytest.mark.parametrize("N,CP,mu", GEOMETRIES)
def test_default_sync_frames_equals_fp64_kernel(N, CP, mu, dt):
    """Clean, noisy, chirp-in-noise, noise-only, silent and NaN-carrying windows (floating storage: int16 cannot hold a NaN),
    a window that starts before the buffer and one that hangs over its end: auto == mode 0.  The clean set goes the screened
    way; want_peak asks for fp64 values and gets the fp64 kernel, values unchanged."""
    p = _params(N, CP, mu)
    clean = _rows(N, CP, mu)
    F, stride = clean.shape
    rows = clean.copy()
    rs = np.random.RandomState(N + 1)
    rows[2] += 0.05 * rs.randn(stride)                         # a noisy window
    rows[3] += 0.6 * rs.randn(stride)                          # chirp near the noise: extrema around the threshold
    rows[5] = 1e-3 * rs.randn(stride)                          # no chirp at all
    rows[6] = 0.0                                              # silence
    rows[5, -64:] = 0.0
    if dt != torch.int16:
        rows[8, 40] = np.nan                                   # a NaN inside the searched window's taps
        rows[9, stride // 2] = np.nan                          # ... and one deep inside the chirp
    eng = engine_for(p, in_dtype=dt, max_window=320)
    lo, W = -8, 320
    for name, x, nwin in (("clean", _store(clean, dt), F), ("mixed", _store(rows, dt), F + 1)):   # F + 1: the last window lies past the buffer's end but for 8 samples
        auto = eng.sync_frames(x, nwin, stride, lo, lo + W)
        assert eng.sync_frames_last() == dict(path=SCREENED, unresolved_capacity=nwin), name
        ref = eng.sync_frames(x, nwin, stride, lo, lo + W, screened=False)
        assert eng.sync_frames_last()["path"] == FP64
        assert torch.equal(auto, ref), (name, auto, ref)
        if name == "clean":
            assert (ref >= 0).all()
        a2, pk = eng.sync_frames(x, nwin, stride, lo, lo + W, want_peak=True)
        assert eng.sync_frames_last() == dict(path=FP64, unresolved_capacity=0)
        r2, pk0 = eng.sync_frames(x, nwin, stride, lo, lo + W, want_peak=True, screened=False)
        assert torch.equal(a2, ref) and torch.equal(r2, ref)
        assert torch.equal(pk.view(torch.int64), pk0.view(torch.int64))                            # bit for bit (NaN-safe)
        work = eng.sync_frames_workspace(nwin)
        work.fill_(0x5a)
        a3, _ = eng.sync_frames(x, nwin, stride, lo, lo + W, want_peak=True, screened=True, work=work)
        assert torch.equal(a3, ref) and int(work[:4].view(torch.int32).item()) == 0               # the fallback zeroes the count word
    with pytest.raises(ValueError, match="work"):
        eng.sync_frames(x, nwin, stride, lo, lo + W, screened=True, work=eng.sync_frames_workspace(nwin)[:-4])


def test_window_wider_than_the_screen_takes_the_fp64_kernel():
    g = load("g3_n4096_16qam_gr5")
    p = params_of(g)
    eng = engine_for(p, max_window=1400)                       # wider than the screen's transform allows
    x = torch.from_numpy(g["r"]).cuda()
    lo = int(g["peaks"][0]) + 1 - (p.Lc - 1) - 600
    auto = eng.sync_frames(x, 1, 0, lo, lo + 1400)
    assert eng.sync_frames_last() == dict(path=FP64, unresolved_capacity=0)
    assert torch.equal(auto, eng.sync_frames(x, 1, 0, lo, lo + 1400, screened=False)) and int(auto[0]) >= 0


def _small_batch(F, seed, dt=torch.float32):
    """F windows of the N = 1024 geometry on the device: the ten packets repeated, every row scaled and some rows noisy."""
    base = _rows(1024, 128, 2)
    rs = np.random.RandomState(seed)
    rows = base[rs.randint(0, base.shape[0], F)] * rs.uniform(0.3, 1.0, (F, 1))
    noisy = rs.rand(F) < 0.3
    rows[noisy] += 0.6 * rs.randn(int(noisy.sum()), base.shape[1])
    rows[rs.rand(F) < 0.05] = 0.0
    return _store(rows, dt), base.shape[1]


def test_library_workspace_grows_and_is_kept_per_stream():
    p = _params(1024, 128, 2)
    eng = engine_for(p, in_dtype=torch.float32, max_window=320)
    xs, stride = _small_batch(16, 1)
    xl, _ = _small_batch(700, 2)
    for x, F in ((xs, 16), (xl, 700), (xs, 16), (xl, 699)):    # first use, growth, the larger workspace on a small call, no growth
        auto = eng.sync_frames(x, F, stride, -8, 312)
        assert eng.sync_frames_last() == dict(path=SCREENED, unresolved_capacity=F)
        assert torch.equal(auto, eng.sync_frames(x, F, stride, -8, 312, screened=False)), F
    # two host threads, each on a stream of its own, different inputs: each gets its own answers
    inputs = [_small_batch(300, 3)[0], _small_batch(450, 4)[0]]
    want = [eng.sync_frames(x, x.shape[0], stride, -8, 312, screened=False).cpu() for x in inputs]
    assert not torch.equal(want[0][:300], want[1][:300])
    got, errs, go = [None, None], [None, None], threading.Barrier(2)
    torch.cuda.synchronize()

    def run(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                go.wait()
                for _ in range(3):
                    got[i] = eng.sync_frames(inputs[i], inputs[i].shape[0], stride, -8, 312)
                    assert eng.sync_frames_last()["path"] == SCREENED
                torch.cuda.current_stream().synchronize()
                got[i] = got[i].cpu()
        except BaseException as e:                             # noqa: BLE001 (reported below)
            errs[i] = e

    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th: t.start()
    for t in th: t.join()
    assert errs == [None, None], errs
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_eight_chunk_pattern_on_a_side_stream_equals_one_fp64_call():
    """The multi-GPU step's sync: slices of one batch, one side stream, per-chunk outputs, chunk-relative offsets."""
    p = _params(1024, 128, 2)
    eng = engine_for(p, in_dtype=torch.float32, max_window=320)
    chunks, Fc = 8, 40
    F = chunks * Fc
    big, stride = _small_batch(F, 5)
    whole = eng.sync_frames(big, F, stride, -8, 312, screened=False)
    starts_c = torch.empty((chunks, Fc), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream(priority=-1)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for c in range(chunks):
            eng.sync_frames(big[c * Fc:(c + 1) * Fc], Fc, stride, -8, 312, out_starts=starts_c[c])
            assert eng.sync_frames_last() == dict(path=SCREENED, unresolved_capacity=Fc)
    torch.cuda.current_stream().wait_stream(side)
    base = (torch.arange(chunks, device="cuda", dtype=torch.int64) * (Fc * stride))[:, None]
    got = torch.where(starts_c >= 0, starts_c + base, starts_c).view(-1)
    assert torch.equal(got, whole)


def test_fp64_pass_resolves_a_long_list_and_an_empty_one():
    """4 096 windows of which a known share is left to the fp64 kernel: more of them than any grid of a few workgroups per
    CU (silent windows: the bound cannot tell their maximum from zero; chirps in noise at the threshold; noise alone), the
    rest clean.  Offsets == mode 0, twice on the same stream (the second call finds the workspace as the first left it); and
    a batch whose list is empty."""
    p = _params(1024, 128, 2)
    K = p.K
    eng = engine_for(p, in_dtype=torch.float32, max_window=320)
    F, stride = 4096, 13056
    gen = torch.Generator(device="cuda").manual_seed(5)
    packed = torch.randint(0, 256, (F, eng.bytes_per_frame), dtype=torch.uint8, device="cuda", generator=gen)
    gaps = torch.randint(0, 300, (F,), dtype=torch.int64, device="cuda", generator=gen)
    filler = np.zeros(K, dtype=complex); filler[K - 1] = (1 - 1j) / np.sqrt(2)
    clean = eng.tx_frames(packed, filler, stride=stride, gaps=gaps, out_dtype=torch.float32)
    rows = clean.clone()
    kind = torch.arange(F, device="cuda") % 8                  # 0-1 clean, 2-4 silent, 5-6 chirp in noise at the threshold, 7 noise alone
    rows[(kind >= 2) & (kind <= 4)] = 0.0
    rows[kind == 7] = 0.0
    noisy = kind >= 5
    rows[noisy] += 0.6 * torch.randn((int(noisy.sum()), stride), device="cuda", generator=gen)
    d = eng.debug_frames_screen(rows, F, stride, -8, 312)
    n_unres = int(d["unresolved"].numel())
    print("windows left to the fp64 kernel:", n_unres, "of", F)
    assert 3 * F // 8 <= n_unres <= F - F // 4                 # at least the silent ones, at most all but the clean ones
    assert n_unres > 4 * torch.cuda.get_device_properties(0).multi_processor_count
    ref = eng.sync_frames(rows, F, stride, -8, 312, screened=False)
    for _ in range(2):
        out = torch.full((F,), -7, dtype=torch.int64, device="cuda")
        eng.sync_frames(rows, F, stride, -8, 312, out_starts=out)
        assert eng.sync_frames_last()["path"] == SCREENED
        assert torch.equal(out, ref)
    work = eng.sync_frames_workspace(F)
    assert torch.equal(eng.sync_frames(rows, F, stride, -8, 312, screened=True, work=work), ref)
    assert int(work[:4].view(torch.int32).item()) == n_unres
    # the empty list: every window decided by the screen, right after a call that left a long one
    assert eng.debug_frames_screen(clean, F, stride, -8, 312)["unresolved"].numel() == 0
    exp = torch.arange(F, device="cuda") * stride + gaps + p.Lc
    assert torch.equal(eng.sync_frames(clean, F, stride, -8, 312), exp)
    assert torch.equal(eng.sync_frames(clean, F, stride, -8, 312, screened=False), exp)
