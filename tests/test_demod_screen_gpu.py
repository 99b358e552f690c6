"""The screened QPSK demodulation (gf3_demod_frames_px, Engine.demod_frames(precision=None | "screen")): data-symbol
transforms in fp32 under a proven bound, the fp64 kernel on the packets the bound cannot decide.  Every equality check
compares with precision="fp64" (the all-fp64 kernel on every packet) bit for bit; the bound checks compare the screen's
fp32 symbols with the fp64 kernel's own dumps."""
import functools

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import tables
from tests.util import engine_for, load

pytestmark = pytest.mark.gpu

SCREENED, FP64 = 0, 2                                              # gf3_demod_frames_last paths
WANT = ("Hs", "He", "slope", "status")

# name -> (N, P, D, F, carrier map or None for the whole band)
GEOMETRIES = {
    "n1024": (1024, 2, 8, 32, None),
    "n2048": (2048, 2, 8, 32, None),
    "n4096": (4096, 2, 8, 32, None),
    "n8192": (8192, 2, 8, 8, None),
    "n1024-scattered": (1024, 2, 8, 32, "scattered"),             # the a.pos branch, C odd
    "n1024-band": (1024, 2, 8, 32, "band"),                       # a band-limited signal: nothing outside the data band
    "n1024-p1d3": (1024, 1, 3, 32, None),
}


def _params(name, table=None):
    N, P, D, F, mp = GEOMETRIES[name]
    K = N // 2 - 1
    pts, bt = table or orc.qpsk_table()
    mu = bt.shape[1]
    known = load("g6_realrec")["known_bits"]
    known = np.tile(known, -(-K * mu // len(known)))
    carriers = None
    if mp == "scattered":
        carriers = tables.shuffled(K)[:-1]
        assert len(carriers) % 2 == 1
    elif mp == "band":
        carriers = tables.contig(K)
    return orc.RxParams(N=N, CP=N // 8, P=P, D=D, lo=1, hi=K, const_points=pts, const_bits=bt, known_bits=known,
                        fit_lo=min(500, K // 2), fit_hi=min(1000, K), carriers=carriers)


@functools.lru_cache(maxsize=None)
def _clean(name, qam16=False):
    """(p, F packets back to back as one fp64 stream, first-pilot offsets)."""
    p = _params(name, orc.square_qam_table(4) if qam16 else None)
    F = GEOMETRIES[name][3]
    rs = np.random.RandomState(len(name) * 131 + p.N)
    payload = rs.randint(0, 2, F * p.D * p.C * p.mu)
    fill = rs.choice(tables.QPSK_FILL, size=p.K - p.C)
    if GEOMETRIES[name][4] == "band":
        fill = np.zeros(p.K - p.C, dtype=complex)
    frames = np.asarray(orc.tx_frames(payload, fill, p), dtype=np.float64)
    assert frames.shape == (F, p.frame_len)
    starts = np.arange(F, dtype=np.int64) * p.frame_len + p.Lc
    return p, frames.reshape(-1).copy(), starts


def _awgn(x, snr_db, seed, p):
    """White noise at snr_db below the OFDM symbols' power (the chirp in front of each packet is several times louder and
    is left out of the reference level)."""
    rs = np.random.RandomState(seed)
    sym = x[p.Lc: p.frame_len]
    return x + rs.randn(len(x)) * np.sqrt(np.mean(sym * sym)) * 10.0 ** (-snr_db / 20.0)


def _store(x, storage):
    """The samples as the storage holds them, on the device (non-finite values survive only in float32)."""
    if storage == "f32":
        return torch.from_numpy(x.astype(np.float32)).cuda()
    fin = np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
    if storage == "i16":
        return torch.from_numpy(np.round(fin * (20000.0 / np.abs(fin).max())).astype(np.int16)).cuda()
    return torch.from_numpy(np.clip(np.round(128.0 + fin * (100.0 / np.abs(fin).max())), 0, 255).astype(np.uint8)).cuda()


DTYPES = dict(f32=torch.float32, i16=torch.int16, u8=torch.uint8, f64=torch.float64)


@functools.lru_cache(maxsize=None)
def _engine(name, storage, qam16=False):
    return engine_for(_clean(name, qam16)[0], in_dtype=DTYPES[storage])


def _bits_of(t):
    """Bit patterns, so that NaN compares equal to itself."""
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b, what, rows=slice(None)):
    """rows: the packets whose Hs / He / slope are compared (a ragged packet's are not written by either path)."""
    for k in ("bits",) + WANT:
        sl = rows if k in ("Hs", "He", "slope") else slice(None)
        assert torch.equal(_bits_of(a[k][sl]), _bits_of(b[k][sl])), (what, k)


def _demod(eng, x, starts, **kw):
    """The one-launch form, whatever the library's own choice between it and the two-phase form would be at this F and D
    (the two-phase form is never screened: test_paths_the_screen_does_not_take)."""
    return eng.demod_frames(x, starts, split=False, **kw)


def _both(eng, x, starts, what, expect_path=SCREENED, rows=slice(None)):
    auto = _demod(eng, x, starts, want=WANT)
    assert eng.demod_frames_last() == dict(path=expect_path, listed_capacity=len(starts) if expect_path == SCREENED else 0), what
    ref = _demod(eng, x, starts, want=WANT, precision="fp64")
    assert eng.demod_frames_last() == dict(path=FP64, listed_capacity=0), what
    _same(auto, ref, what, rows)
    return auto, ref


def _sym(p, f, l):
    """Sample range of data symbol l of packet f in the back-to-back stream (prefix included)."""
    s0 = f * p.frame_len + p.Lc + (p.P + l) * (p.N + p.CP)
    return slice(s0, s0 + p.N + p.CP)


@pytest.mark.parametrize("storage", ["f32", "i16", "u8"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_screened_demod_equals_fp64_kernel(name, storage):
    """Clean, 20 dB, 3 dB (many packets listed: the list and the fp64 pass), the multipath fixture's channel, a silent data
    symbol, NaN / Inf in a data symbol and in a pilot (float storage), a ragged first and last packet: auto == fp64 on bits,
    Hs, He, slope and status.  Clean and 20 dB list nothing; every packet with a silent or non-finite symbol is listed."""
    p, x0, starts = _clean(name)
    F = len(starts)
    eng = _engine(name, storage)
    seed = len(name) + p.N
    for what, x in (("clean", x0), ("awgn20", _awgn(x0, 20.0, seed, p))):
        xs = _store(x, storage)
        _both(eng, xs, starts, what)
        dbg = eng.debug_demod_screen(xs, starts)
        assert int(dbg["cls"].sum()) == 0 and dbg["listed"].numel() == 0, (what, dbg["listed"])
        assert torch.equal(dbg["bits"], _demod(eng, xs, starts, precision="fp64")["bits"]), what
    xs = _store(_awgn(x0, 3.0, seed + 1, p), storage)
    _both(eng, xs, starts, "awgn3")
    n3 = int(eng.debug_demod_screen(xs, starts)["cls"].sum())
    h = load("g3_n4096_16qam_gr5")["channel"]
    _both(eng, _store(_awgn(np.convolve(x0, h)[: len(x0)], 30.0, seed + 2, p), storage), starts, "multipath")
    # a silent data symbol in packets 1 and F - 2: every part is +-0 (u8 storage: the constant 128 -- DC only)
    x = x0.copy()
    quiet = [1, F - 2]
    for f in quiet:
        x[_sym(p, f, p.D - 1)] = 0.0
    xs = _store(x, storage)
    _both(eng, xs, starts, "silent")
    dbg = eng.debug_demod_screen(xs, starts)
    assert dbg["listed"].tolist() == quiet and dbg["cls"].nonzero().flatten().tolist() == quiet
    if storage == "f32":
        x = x0.copy()
        x[_sym(p, 0, 0).start + p.CP + 5] = np.nan              # a data symbol's own samples
        x[_sym(p, 2, p.D - 1).start + p.CP + 6] = np.inf
        x[3 * p.frame_len + p.Lc + p.CP + 7] = np.nan            # a start pilot
        x[_sym(p, 4, p.D).start + p.CP + 8] = -np.inf            # an end pilot
        xs = _store(x, storage)
        _both(eng, xs, starts, "nonfinite")
        assert eng.debug_demod_screen(xs, starts)["listed"].tolist() == [0, 2, 3, 4]
    # ragged: the first packet starts before the buffer, the last one hangs over its end
    rag = starts.copy()
    rag[0] = -1
    xs = _store(x0[: len(x0) - 3], storage)
    auto, _ = _both(eng, xs, rag, "ragged", rows=slice(1, F - 1))
    assert int(auto["status"].item()) == 1 and not auto["bits"][0].any() and not auto["bits"][-1].any()
    assert eng.debug_demod_screen(xs, rag)["listed"].numel() == 0          # ragged packets are not listed
    print(f"{name} {storage}: listed at 3 dB {n3} of {F}")


def test_paths_the_screen_does_not_take():
    """f64 storage, eq asked for, the two-phase form, a 16-QAM table: all fp64 (path 2), outputs those of precision="fp64"."""
    name = "n1024"
    p, x0, starts = _clean(name)
    x = _awgn(x0, 20.0, 5, p)
    eng64 = _engine(name, "f64")
    _both(eng64, torch.from_numpy(x).cuda(), starts, "f64 storage", expect_path=FP64)
    eng = _engine(name, "f32")
    xs = _store(x, "f32")
    a = _demod(eng, xs, starts, want=("eq",))
    assert eng.demod_frames_last()["path"] == FP64
    b = _demod(eng, xs, starts, want=("eq",), precision="fp64")
    assert torch.equal(a["bits"], b["bits"]) and torch.equal(_bits_of(a["eq"]), _bits_of(b["eq"]))
    a = eng.demod_frames(xs, starts, split=True)
    assert eng.demod_frames_last()["path"] == FP64
    assert torch.equal(a["bits"], eng.demod_frames(xs, starts, split=True, precision="fp64")["bits"])
    assert torch.equal(a["bits"], _demod(eng, xs, starts)["bits"])
    assert eng.demod_frames_last()["path"] == SCREENED
    p16, x16, s16 = _clean(name, True)
    _both(_engine(name, "f32", True), _store(_awgn(x16, 30.0, 6, p16), "f32"), s16, "16-QAM", expect_path=FP64)
    with pytest.raises(ValueError, match="precision"):
        _demod(eng, xs, starts, precision="fp32")


def test_capture_without_a_workspace_takes_the_fp64_kernel():
    """Nothing is allocated while the stream is being captured: a first call under capture runs all fp64, and so does its
    replay; the same call outside the capture then gets a workspace and is screened."""
    name = "n1024"
    p, x0, starts = _clean(name)
    eng = engine_for(p, in_dtype=torch.float32)                   # a fresh context: no workspace yet
    xs = _store(x0, "f32")
    off = torch.from_numpy(starts).cuda()
    bits = torch.zeros((len(starts), eng.bytes_per_frame), dtype=torch.uint8, device="cuda")
    ref = torch.zeros_like(bits)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        _demod(eng, xs, off, out_bits=ref, precision="fp64")
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            _demod(eng, xs, off, out_bits=bits)
            last = eng.demod_frames_last()
        graph.replay()
        side.synchronize()
        assert last == dict(path=FP64, listed_capacity=0)
        assert torch.equal(bits, ref)
        bits.zero_()
        _demod(eng, xs, off, out_bits=bits)
        assert eng.demod_frames_last()["path"] == SCREENED
        side.synchronize()
        assert torch.equal(bits, ref)
    torch.cuda.current_stream().wait_stream(side)


def test_workspace_is_kept_per_stream_next_to_the_syncs():
    """Sync and demodulation queued on one stream keep separate lists; two streams keep separate workspaces."""
    name = "n1024"
    p, x0, starts = _clean(name)
    eng = engine_for(p, in_dtype=torch.float32, max_window=320)
    xs = _store(_awgn(x0, 3.0, 9, p), "f32")
    ref = _demod(eng, xs, starts, precision="fp64")["bits"]
    F = len(starts)
    sync_ref = eng.sync_frames(xs, F, p.frame_len, -8, 312, screened=False)
    outs = []
    for _ in range(2):
        with torch.cuda.stream(torch.cuda.Stream()):
            for n in (F // 2, F):                                  # first use, growth
                st = eng.sync_frames(xs, F, p.frame_len, -8, 312)
                o = _demod(eng, xs, starts[:n])
                assert eng.demod_frames_last() == dict(path=SCREENED, listed_capacity=n)
                outs.append((n, o["bits"], st))
            torch.cuda.current_stream().synchronize()
    for n, b, st in outs:
        assert torch.equal(b, ref[:n]) and torch.equal(st, sync_ref)


# ---- the bound ------------------------------------------------------------------------------------------------------
BOUND_INPUTS = ["clean", "noisy", "dc", "i16-full-scale", "dominant-carrier", "impulse"]


def _bound_input(kind, p, x0, F):
    x = x0.copy()
    if kind == "noisy":
        x = _awgn(x, 10.0, 3, p)
    elif kind == "dc":
        x = x + 0.5 * np.abs(x).max()
    elif kind == "dominant-carrier":                               # one data carrier 10^6 times the others, over the whole stream
        k = int(p.data_carriers[len(p.data_carriers) // 3])
        amp = 2.0 * np.sqrt(np.mean(x * x) / p.C)                  # about one carrier's time-domain amplitude
        x = x + 1e6 * amp * np.cos(2 * np.pi * k * np.arange(len(x)) / p.N + 0.3)
    elif kind == "impulse":                                        # one non-zero sample per symbol: |x|_1 as small as it gets
        for f in range(F):
            sl = _sym(p, f, f % p.D)
            x[sl] = 0.0
            x[sl.start + p.CP + (37 * f + (f & 1)) % p.N] = 1.0
    return x


@pytest.mark.parametrize("name", ["n1024", "n2048", "n4096", "n8192", "n1024-scattered"])
def test_bound_holds_with_a_factor_of_two(name):
    """max |ep32 - ep64| over the data carriers of a symbol <= E_l / 2, ep64 = 2 eq |Hest| from the fp64 kernel's dumps (the
    kernel's transforms leave 2 X: exact to ~1e-15).  Prints the worst realised ratio per input."""
    p, x0, starts = _clean(name)
    F = min(len(starts), 8)
    starts = starts[:F]
    x0 = x0[: F * p.frame_len]
    cols = torch.from_numpy(np.asarray(p.data_carriers) - 1).cuda()
    worst = {}
    for kind in BOUND_INPUTS:
        storage = "i16" if kind == "i16-full-scale" else "f32"
        x = _bound_input(kind, p, x0, F)
        if storage == "i16":
            xs = torch.from_numpy(np.round(x * (32767.0 / np.abs(x).max())).astype(np.int16)).cuda()
        else:
            xs = _store(x, storage)
        eng = _engine(name, storage)
        full = _demod(eng, xs, starts, want=("eq", "Hest"))
        ep64 = 2.0 * full["eq"].reshape(F, p.D, p.C) * full["Hest"][:, :, cols].abs()
        dbg = eng.debug_demod_screen(xs, starts)
        err = (dbg["ep32"].to(torch.complex128) - ep64).abs().amax(dim=2)          # [F, D]
        E = dbg["E"].to(torch.float64)
        assert torch.isfinite(E).all() and (E > 0).all(), kind
        ratio = float((err / E).max())
        worst[kind] = ratio
        assert ratio <= 0.5, (kind, ratio)
        # the whole path still equals the fp64 kernel on these inputs
        assert torch.equal(_demod(eng, xs, starts)["bits"], _demod(eng, xs, starts, precision="fp64")["bits"]), kind
    print(f"{name}: worst |ep32 - ep64| / E_l: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---- the fp32 transform alone ---------------------------------------------------------------------------------------
STAGE_SUM = {512: 248.0, 1024: 184.0, 2048: 272.0, 4096: 360.0}    # gf3rx_dscreen.h: sum of the stage constants, in units of 2^-24


@pytest.mark.parametrize("storage", ["f32", "i16"])
@pytest.mark.parametrize("name", ["n1024", "n2048", "n4096", "n8192"])
def test_fp32_transform_alone_against_numpy(name, storage):
    """Every bin 0 .. N/2 of rfft_regs<.., float2> (DC and Nyquist from z0, the non-data bins too) against numpy's fp64 rfft
    of the same stored samples, at offsets of both parities: |X32 - X| <= half the header's bound on X (GAMMA / 2 on the
    symbol's l1 norm: GAMMA bounds 2 X), on a packet's symbols, on noise and on an impulse."""
    p, x0, starts = _clean(name)
    N, NC = p.N, p.N // 2
    rs = np.random.RandomState(N)
    x = x0[: p.frame_len + 8].copy()
    x[:N] = rs.randn(N)                                          # white noise
    x[N: 2 * N] = 0.0
    x[N + 77] = 1.0                                              # an impulse
    xs = _store(x, storage)
    offs = np.array([0, N, p.Lc + p.CP, p.Lc + p.CP + 1, p.Lc + 3 * (N + p.CP) + 5], dtype=np.int64)
    got = _engine(name, storage).debug_rfft32_batch(xs, offs).cpu().numpy().astype(np.complex128)
    xh = xs.cpu().numpy().astype(np.float64)
    gamma_x = 0.5 * 2.0 * 2.0 * np.sqrt(2.0) * STAGE_SUM[NC] * 2.0 ** -24
    worst = 0.0
    for i, o in enumerate(offs):
        seg = xh[o: o + N]
        err = np.abs(got[i] - np.fft.rfft(seg)).max()
        bound = gamma_x * np.abs(seg).sum()
        worst = max(worst, err / bound)
        assert err <= 0.5 * bound, (int(o), err, bound)
    print(f"{name} {storage}: worst |X32 - X| / bound {worst:.2e}")
