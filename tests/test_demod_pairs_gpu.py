"""The screened QPSK demodulation (gf3rx_dscreen.h), which transforms its data symbols two at a time, where that data
loop can go wrong: every parity of D, decision rings whose words span several symbols, symbols of very different level
sharing a transform, the pair transform alone against numpy, and the fp32 phasor recurrence over a long packet.  Every equality check compares with precision="fp64" (the all-fp64 kernel on every packet) bit for
bit; the bound check compares the screen's fp32 symbols with the fp64 kernel's own MODE_FULL dumps.

Every stream carries a sampling-clock drift (each symbol circularly delayed by a little more than the one before), so
that the fitted phase slope is far from zero and the per-symbol phasor step is a real rotation: on an undrifted stream
gstep is 1 to rounding and the recurrence is exercised by nothing."""
import functools

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import tables
from tests.test_demod_screen_gpu import DTYPES, FP64, SCREENED, STAGE_SUM, _awgn, _both, _demod, _store, _sym
from tests.test_demod_screen_gpu import _clean as _screen_clean
from tests.util import engine_for, load

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SIZES = [1024, 2048, 4096, 8192]
DRIFT = 0.02                                                       # samples per symbol


def _frames_of(N):
    return 8 if N == 8192 else 32


def _params(N, P, D, carriers=None, **kw):
    K = N // 2 - 1
    pts, bt = orc.qpsk_table()
    known = load("g6_realrec")["known_bits"]
    known = np.tile(known, -(-K * 2 // len(known)))
    if carriers is None and "lo" not in kw:
        kw.update(lo=1, hi=K)
    kw.setdefault("CP", N // 8)
    kw.setdefault("fit_lo", min(500, K // 2))
    kw.setdefault("fit_hi", min(1000, K))
    return orc.RxParams(N=N, P=P, D=D, const_points=pts, const_bits=bt, known_bits=known, carriers=carriers, **kw)


def _drift(frames, p, delta):
    """Symbol i of every packet (pilots included) circularly delayed by i * delta samples, exactly (a phase ramp over its
    spectrum; the prefix rebuilt): what a slow receiver clock does to a packet, without the interpolation noise."""
    out = frames.copy()
    S = p.N + p.CP
    n = np.fft.rfftfreq(p.N, 1.0 / p.N)
    for i in range(2 * p.P + p.D):
        body = out[:, p.Lc + i * S + p.CP: p.Lc + (i + 1) * S]
        spec = np.fft.rfft(body, axis=1) * np.exp(-2j * np.pi * n * (i * delta) / p.N)
        spec[:, -1] = spec[:, -1].real
        d = np.fft.irfft(spec, p.N, axis=1)
        out[:, p.Lc + i * S + p.CP: p.Lc + (i + 1) * S] = d
        if p.CP:
            out[:, p.Lc + i * S: p.Lc + i * S + p.CP] = d[:, -p.CP:]
    return out


@functools.lru_cache(maxsize=None)
def _stream(N, P, D, cmap=None, F=None, mode_a2=False):
    """(p, F drifted packets back to back as one fp64 stream, first-pilot offsets).  cmap: None (the whole band) or
    (C, "band" | "scattered")."""
    K = N // 2 - 1
    carriers = None
    if cmap is not None:
        C, kind = cmap
        if kind == "band":
            carriers = np.arange(K // 5 + 1, K // 5 + 1 + C) if C < K - K // 5 else np.arange(1, C + 1)
        else:
            carriers = np.random.RandomState(C).permutation(np.arange(2, K))[:C]
    p = _params(N, P, D, CP=224, lo=100, hi=1500) if mode_a2 else _params(N, P, D, carriers)
    F = F or _frames_of(N)
    rs = np.random.RandomState(N + 8 * D + P + (0 if cmap is None else 131 * cmap[0]))
    payload = rs.randint(0, 2, F * p.D * p.C * p.mu)
    fill = rs.choice(tables.QPSK_FILL, size=p.K - p.C)
    frames = _drift(np.asarray(orc.tx_frames(payload, fill, p), dtype=np.float64), p, DRIFT)
    starts = np.arange(F, dtype=np.int64) * p.frame_len + p.Lc
    return p, frames.reshape(-1).copy(), starts


def _store16(x):
    """int16 at full scale (tests whose quietest symbols sit three orders under the loudest)."""
    return torch.from_numpy(np.round(x * (32767.0 / np.abs(x).max())).astype(np.int16)).cuda()


def _screened_nothing_listed(eng, xs, starts, what):
    dbg = eng.debug_demod_screen(xs, starts)
    assert int(dbg["cls"].sum()) == 0 and dbg["listed"].numel() == 0, (what, dbg["listed"].tolist())
    return dbg


@pytest.mark.parametrize("storage", ["f32", "i16"])
@pytest.mark.parametrize("N", SIZES)
def test_every_parity_of_d(N, storage):
    """D in {1, 2, 5, 6} x P in {1, 2}: auto == fp64 on bits, Hs, He, slope and status, clean (nothing listed: the bits are
    fp32 decisions) and at 3 dB (the list and the fp64 pass)."""
    for D in (1, 2, 5, 6):
        for P in (1, 2):
            p, x0, starts = _stream(N, P, D)
            eng = engine_for(p, in_dtype=DTYPES[storage])
            xs = _store(x0, storage)
            what = (N, storage, D, P)
            _both(eng, xs, starts, what + ("clean",))
            _screened_nothing_listed(eng, xs, starts, what)
            _both(eng, _store(_awgn(x0, 3.0, N + D + P, p), storage), starts, what + ("awgn3",))


# (N, C, map): C mu = 14 (a word spans three symbols), 34 (just over a word), 32 and 2048 (whole words), 4092 (the
# headline's straddle); N >= 2048 has more than one wave per workgroup
RING_CASES = [(1024, 7, "band"), (2048, 7, "band"), (2048, 17, "scattered"), (2048, 16, "band"), (4096, 7, "scattered"),
              (4096, 17, "band"), (4096, 16, "scattered"), (4096, 1024, "band"), (4096, 2046, "band"), (8192, 17, "band")]


@pytest.mark.parametrize("storage", ["f32", "i16"])
@pytest.mark.parametrize("N,C,kind", RING_CASES, ids=[f"n{n}-c{c}-{k}" for n, c, k in RING_CASES])
def test_decision_ring(N, C, kind, storage):
    """D = 5 and D = 6: every output byte equals the fp64 path's, nothing is listed (so the bytes come from the screen's
    ring), and the call repeated 20 times gives the same bytes each time -- a slot overwritten while it is still being
    packed is a race, and one run proves little.
    Listed on these clean inputs by the parent commit's screen (fp64 phasors), checked before this test was written:
    0 of F in every case and storage."""
    for D in (5, 6):
        p, x0, starts = _stream(N, 2, D, (C, kind))
        assert p.C == C
        eng = engine_for(p, in_dtype=DTYPES[storage])
        xs = _store(x0, storage)
        what = (N, C, kind, storage, D)
        auto, _ = _both(eng, xs, starts, what)
        _screened_nothing_listed(eng, xs, starts, what)
        first = auto["bits"].clone()
        for rep in range(20):
            again = _demod(eng, xs, starts)["bits"]
            assert eng.demod_frames_last()["path"] == SCREENED
            assert torch.equal(again, first), what + (rep,)


@pytest.mark.parametrize("storage", ["f32", "i16"])
@pytest.mark.parametrize("N", SIZES)
def test_neighbouring_symbols_do_not_mix(N, storage):
    """Data symbols alternating x1, x1000, x1, ... and, in two packets, a silent odd symbol: E[f, l] is GAMMA |x_l|_1
    (1 + 1e-3) of that symbol's OWN samples to 1e-4, only the packets with the silent symbol are listed, auto == fp64."""
    D = 6
    p, x0, starts = _stream(N, 2, D)
    F = len(starts)
    x = x0.copy()
    for f in range(F):
        for l in range(1, D, 2):
            x[_sym(p, f, l)] *= 1000.0
    quiet = {1: 1, F - 2: 3}                                       # packet -> its silent (second-of-pair) symbol
    for f, l in quiet.items():
        x[_sym(p, f, l)] = 0.0
    xs = _store(x, "f32") if storage == "f32" else _store16(x)
    eng = engine_for(p, in_dtype=DTYPES[storage])
    _both(eng, xs, starts, (N, storage))
    dbg = eng.debug_demod_screen(xs, starts)
    assert dbg["listed"].tolist() == sorted(quiet) and dbg["cls"].nonzero().flatten().tolist() == sorted(quiet)
    xh = xs.cpu().numpy().astype(np.float64)
    gamma = 2.0 * 2.0 * np.sqrt(2.0) * STAGE_SUM[N // 2] * U
    want = np.empty((F, D))
    for f in range(F):
        for l in range(D):
            sl = _sym(p, f, l)
            want[f, l] = gamma * np.abs(xh[sl.start + p.CP: sl.stop]).sum() * 1.001 + 1e-30
    got = dbg["E"].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - want) <= 1e-4 * want), float(np.abs(got / want - 1.0).max())


@pytest.mark.parametrize("storage", ["f32", "i16"])
@pytest.mark.parametrize("N", SIZES)
def test_pair_transform_alone_against_numpy(N, storage):
    """Every bin 0 .. N/2 of rfft_regs<.., cf2> -- the instantiation the screen runs on its data symbols, two symbols per
    workgroup -- against numpy's fp64 rfft of the same stored samples, for n_sym = 1, 2 and 7 (an absent second half, a whole
    pair, both): |X32 - X| <= half the header's bound on X.  Inputs and constant are those of
    tests/test_demod_screen_gpu.py::test_fp32_transform_alone_against_numpy (a packet's symbols at offsets of both
    parities, white noise, an impulse)."""
    p, x0, starts = _screen_clean({1024: "n1024", 2048: "n2048", 4096: "n4096", 8192: "n8192"}[N])
    NC = N // 2
    rs = np.random.RandomState(N)
    x = x0[: p.frame_len + 8].copy()
    x[:N] = rs.randn(N)                                          # white noise
    x[N: 2 * N] = 0.0
    x[N + 77] = 1.0                                              # an impulse
    xs = _store(x, storage)
    xh = xs.cpu().numpy().astype(np.float64)
    all_offs = np.array([0, N, p.Lc + p.CP, p.Lc + p.CP + 1, p.Lc + 3 * (N + p.CP) + 5, N, 0], dtype=np.int64)
    gamma_x = 0.5 * 2.0 * 2.0 * np.sqrt(2.0) * STAGE_SUM[NC] * 2.0 ** -24
    eng = engine_for(p, in_dtype=DTYPES[storage])
    worst = 0.0
    for n_sym in (1, 2, 7):
        offs = all_offs[-n_sym:] if n_sym < 7 else all_offs      # (1: the noise alone; 2: the impulse beside the noise)
        got = eng.debug_rfft32_pair_batch(xs, offs).cpu().numpy().astype(np.complex128)
        assert got.shape == (n_sym, NC + 1)
        for i, o in enumerate(offs):
            seg = xh[o: o + N]
            err = np.abs(got[i] - np.fft.rfft(seg)).max()
            bound = gamma_x * np.abs(seg).sum()
            worst = max(worst, err / bound)
            assert err <= 0.5 * bound, (n_sym, int(o), err, bound)
    print(f"n{N} {storage}: worst |X32 - X| / bound {worst:.2e}")


def test_phasor_bound_over_a_long_packet():
    """Mode A2's shape (N = 4096, P = 20, D = 180, carriers 100 .. 1500; F = 3), one launch: for every data carrier of every
    symbol |ep32 - ep64| <= (E_l + C_l u (|ep32.x| + |ep32.y|)) / 2 with C_l = 8 + 8 (l + 1) (gf3rx_dscreen.h, "The
    rotation"), ep64 = 2 eq |Hest| from the fp64 kernel's dumps; and auto == fp64 bit for bit, nothing listed.  Prints the
    worst realised ratio and where the fp32 phasors stand at the last symbol."""
    p, x0, starts = _stream(4096, 20, 180, F=3, mode_a2=True)
    F = len(starts)
    xs = _store(x0, "f32")
    eng = engine_for(p, in_dtype=torch.float32)
    _both(eng, xs, starts, "A2")
    dbg = _screened_nothing_listed(eng, xs, starts, "A2")
    full = _demod(eng, xs, starts, want=("eq", "Hest", "slope"))
    assert eng.demod_frames_last()["path"] == FP64
    assert float(full["slope"].abs().min()) > 1e-4                 # the phasors do turn
    cols = torch.from_numpy(np.asarray(p.data_carriers) - 1).cuda()
    ep64 = 2.0 * full["eq"].reshape(F, p.D, p.C) * full["Hest"][:, :, cols].abs()
    ep32 = dbg["ep32"]
    err = (ep32.to(torch.complex128) - ep64).abs()                 # [F, D, C]
    Cl = 8.0 + 8.0 * torch.arange(1, p.D + 1, dtype=torch.float64, device="cuda")
    l1part = (ep32.real.abs() + ep32.imag.abs()).to(torch.float64)
    bound = dbg["E"].to(torch.float64)[:, :, None] + (Cl * U)[None, :, None] * l1part
    ratio = err / bound
    rot = (err / l1part)[:, -1].max() / U                          # everything, the transform's error too, in u of the symbol
    print(f"A2: worst |ep32 - ep64| / (E_l + C_l u |ep32|_1) {float(ratio.max()):.2e}; at l = D - 1: {float(rot):.0f} u, C_l = {float(Cl[-1]):.0f}")
    assert float(ratio.max()) <= 0.5
