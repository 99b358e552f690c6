"""gf3_detect_chunk / gf3_detect_decide (the self-normalised chirp detection) against the NumPy restatement in
tests/detect_ref.py.  Geometry N = 1024, CP = 128, P = 1, D = 2: Lc = 5760 and frame_len = 10368 < 2 Lc, so neighbouring
chirps' suppression windows nearly touch.  Three packets and a terminating chirp, about 53 000 samples.

Tolerance: |rho_gpu - rho_ref| <= 1e-9 on the lags with V >= 1e-6 max V -- the project's 1e-12 max|P| agreement between
matched-filter forms (test_matched_filter_forms_agree) divided by the smallest normaliser admitted; elsewhere only the
detections are compared."""
import ctypes as C

import numpy as np
import pytest
import torch

from gf3_audio_modem_amd import _lib
from gf3_audio_modem_amd.engine import ListOverflow
from gf3_audio_modem_amd.live import END
from oracle import gf3_oracle as orc
from tests import detect_ref
from tests.util import engine_for, load, params_of

pytestmark = pytest.mark.gpu

TAU = 0.3
P_ = params_of(load("g1_n1024_qpsk"), N=1024, CP=128, P=1, D=2, lo=1, hi=511)
LC, FRAME = P_.Lc, P_.frame_len
LEAD = 8000


def stream(lead=LEAD, gaps=None, tail=8000, seed=1):
    rs = np.random.RandomState(seed)
    bits = rs.randint(0, 2, 3 * P_.D * P_.C * P_.mu)
    fill = orc.qpsk_table()[0][rs.randint(0, 4, P_.K - P_.C)]
    x = orc.tx_stream(bits, fill, P_, gaps=gaps, lead=lead, tail=tail)
    g = np.zeros(3, dtype=int) if gaps is None else np.asarray(gaps)
    starts = lead + np.cumsum(g) + FRAME * np.arange(3)
    chirps = np.append(starts, starts[-1] + FRAME)
    return x, (chirps + LC - 2).astype(np.int64)             # detections: the chirp's last lag g = start + Lc - 1, reported as g - 1


CHIRP = orc.chirp_replica(P_)
_cache = {}


def case(name):
    """-> (samples as stored, expected detections, the restatement's rho and V), made once."""
    if name not in _cache:
        x, want = stream()
        if name == "awgn":
            x = x + np.random.RandomState(2).normal(0.0, np.sqrt(np.mean(CHIRP ** 2)), len(x))
        elif name == "u8":
            x = np.round(128 + 40 * x).astype(np.uint8)
        elif name == "i16":
            x = np.round(20000 * x).astype(np.int16)
        elif name in ("f32", "f32_nan"):                        # the DT_F32 kernels, and det_clean_kernel<float> behind a NaN
            x = x.astype(np.float32)
            if name == "f32_nan":
                x[LEAD + FRAME + LC + 2000] = np.nan
        elif name == "zeros":
            x, want = stream(lead=45000, gaps=[0, 3 * LC, 0])
        elif name == "nan":
            x = x.copy()
            x[LEAD + FRAME + LC + 2000] = np.nan                # inside the second packet's body
        q, V = detect_ref.rho(x, CHIRP)
        assert np.array_equal(detect_ref.detect(q, len(x), LC, TAU), want), name
        _cache[name] = (x, want, q, V)
    return _cache[name]


_engines = {}


def eng_for(x):
    dt = {np.dtype("float64"): torch.float64, np.dtype("float32"): torch.float32, np.dtype("uint8"): torch.uint8,
          np.dtype("int16"): torch.int16}[x.dtype]
    if dt not in _engines:
        _engines[dt] = engine_for(P_, in_dtype=dt)
    return _engines[dt]


def agree(got, q, V, bound, least=3 * FRAME):
    """got vs the restatement where the normaliser is admitted (on more than `least` lags); -> the largest difference there."""
    ok = np.isfinite(V) & (V >= 1e-6 * np.nanmax(V))
    assert ok.sum() > least
    err = np.abs(got[ok] - q[ok]).max()
    print(f"largest |rho_gpu - rho_ref| on {ok.sum()} lags: {err:.3e}")
    assert err <= bound
    return err


@pytest.mark.parametrize("name", ["clean", "awgn", "u8", "i16", "zeros", "nan", "f32", "f32_nan"])
def test_rho_and_detections_match_the_restatement(name):
    x, want, q, V = case(name)
    eng = eng_for(x)
    peaks, got = eng.detect_stream(x, TAU, want_rho=True)
    got = got.cpu().numpy()
    assert np.array_equal(peaks.cpu().numpy(), want)
    agree(got, q, V, 1e-9)
    assert np.array_equal(np.isnan(got), np.isnan(q))         # exactly the windows that hold a sample that is not finite
    at = got[want + 1]
    if name == "clean":
        assert np.abs(at - 1.0).max() < 1e-9
    if name == "awgn":
        assert np.all(np.abs(at - 0.71) < 0.03)
    if name == "zeros":
        r = np.asarray(x)
        csum = np.concatenate([[0], np.cumsum(r != 0)])
        g = np.arange(LC - 1, len(r))
        silent = g[csum[g + 1] - csum[g - LC + 1] == 0]
        assert len(silent) > 45000 - LC + 2 * LC and np.all(got[silent] == 0.0) and np.all(q[silent] == 0.0)
    if name in ("nan", "f32_nan"):
        assert np.isnan(got).sum() == LC


def pieces(eng, x, cuts, LC=LC):
    """The stream through detect_chunk / detect_decide piece by piece (new samples [a, b) per piece, Lc - 1 samples of context in
    front), a decision after every piece -> (detections in the order they were emitted, rho of every lag)."""
    n = len(x)
    dev = eng.device
    xd = eng._samples(x)
    vrun = torch.zeros(1, dtype=torch.float64, device=dev)
    idx = torch.zeros(0, dtype=torch.int64, device=dev)
    rho = torch.zeros(0, dtype=torch.float64, device=dev)
    rho_all = torch.zeros(n + LC - 1, dtype=torch.float64, device=dev)
    found, decided = [], -END
    for a, b in zip(cuts[:-1], cuts[1:]):
        base = max(0, a - (LC - 1))
        mine = torch.zeros(b - base + LC - 1, dtype=torch.float64, device=dev)
        i, r = eng.detect_chunk(xd[base:b], a - base, b - base, base, vrun, TAU, cap=4096, rho_all=mine)
        rho_all[a:b] = mine[a - base: b - base]
        idx, rho = torch.cat([idx, i]), torch.cat([rho, r])
        final = END if b == n else b - 1
        peaks = eng.detect_decide(idx, rho, final).cpu().numpy()
        found += [int(p) for p in peaks if p + LC > decided]   # (the others were emitted before)
        decided = final
    return np.array(found, dtype=np.int64), rho_all.cpu().numpy()


def test_piece_invariance():
    x, want, q, V = case("awgn")
    eng = eng_for(x)
    n = len(x)
    one = eng.detect_stream(x, TAU, want_rho=True)[1].cpu().numpy()
    g = int(want[1]) + 1                                      # the second chirp's peak lag
    cuttings = [list(range(0, n, size)) + [n] for size in (LC + 3, 7001, FRAME)] + [[0, c, n] for c in (g, g - 1, g + 1)]
    for cuts in cuttings:
        found, got = pieces(eng, x, cuts)
        assert np.array_equal(found, want), cuts[:3]
        assert np.abs(got - one).max() <= 2e-9
        agree(got, q, V, 1e-9)


def test_windowed_maximum_rule_on_crafted_lists():
    eng = eng_for(case("clean")[0])

    def decide(idx, rho, final=END, cap=None):
        return eng.detect_decide(np.array(idx, dtype=np.int64), np.array(rho, dtype=np.float64), final, cap).cpu().tolist()
    assert decide([], []) == []
    assert decide([1000, 1000 + LC - 1], [0.5, 0.6]) == [1000 + LC - 1]          # Lc - 1 apart: only the larger
    assert decide([1000, 1000 + LC - 1], [0.6, 0.5]) == [1000]
    assert decide([1000, 1000 + LC], [0.5, 0.6]) == [1000, 1000 + LC]            # Lc apart: both
    assert decide([1000, 1001, 1000 + LC - 1], [0.7, 0.7, 0.7]) == [1000]        # equal: the smaller index
    assert decide([10, 20, 30, 30 + LC], [0.4, 0.9, 0.5, 0.31]) == [20, 30 + LC]
    # a chain: b beats a, c beats b -- a is still no detection (it is not the largest of ITS neighbourhood)
    assert decide([0, LC - 1, 2 * LC - 2], [0.5, 0.6, 0.7]) == [2 * LC - 2]
    # withheld while the neighbourhood reaches final_below, emitted by a later call
    assert decide([1000, 50000], [0.5, 0.6], final=50000 + LC - 1) == [1000]
    assert decide([1000, 50000], [0.5, 0.6], final=50000 + LC) == [1000, 50000]
    # more entries than one step of the kernel, and the capacity
    many = list(range(0, 3000 * LC, LC))
    assert decide(many, [0.5] * len(many)) == many
    with pytest.raises(Exception, match="gf3_detect_decide: 3000 peaks exceed capacity 2999"):
        decide(many, [0.5] * len(many), cap=2999)


def test_overflow_recovery_and_determinism():
    x, want, q, V = case("clean")
    eng = eng_for(x)
    n = len(x)
    full = np.arange(LC - 1, n)
    vrun = torch.zeros(1, dtype=torch.float64, device=eng.device)
    with pytest.raises(ListOverflow, match="gf3_detect_chunk: .* lags to list exceed capacity 4") as e:
        eng.detect_chunk(x, 0, n + LC - 1, 0, vrun, TAU, cap=4)
    assert e.value.wanted == int((q[full] > TAU).sum()) > 4
    assert float(vrun) == 0.0                                 # an overflowing call leaves the running maximum alone
    idx, rho = eng.detect_chunk(x, 0, n + LC - 1, 0, vrun, TAU, cap=e.value.wanted)
    assert np.array_equal(idx.cpu().numpy(), np.flatnonzero(q > TAU) - 1) and float(vrun) > 0.0
    # detect_stream: a threshold low enough to overflow its first list
    low = 0.01
    assert int((q[full] > low).sum()) > 64 * (n // LC + 4)
    assert np.array_equal(eng.detect_stream(x, low).cpu().numpy(), detect_ref.detect(q, n, LC, low))
    a = eng.detect_stream(x, TAU, want_rho=True)[1]
    b = eng.detect_stream(x, TAU, want_rho=True)[1]
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    # the ABI itself: tau outside (0, 1) or not finite is GF3_EINVAL; cap = 0 with no list buffers only counts
    xd = eng._samples(x)
    work = torch.empty(int(eng.lib.gf3_detect_chunk_workspace_bytes(eng._h, n)), dtype=torch.uint8, device=eng.device)
    cnt = C.c_int64(-1)

    def raw(tau):
        return eng.lib.gf3_detect_chunk(eng._h, _lib.ptr(xd), n, 0, n + LC - 1, 0, tau, _lib.ptr(vrun), None, None, 0, C.byref(cnt),
                                        None, _lib.ptr(work), eng._stream())
    for tau in (0.0, 1.0, -0.3, float("nan"), float("inf")):
        assert raw(tau) == _lib.GF3_EINVAL
    assert raw(TAU) == _lib.GF3_ERANGE and cnt.value == e.value.wanted


def test_quiet_second_transmission():
    x, want, _, _ = case("clean")
    eng = eng_for(x)
    both = np.concatenate([x, 0.05 * x])
    assert np.array_equal(eng.sync_stream(both).cpu().numpy(), want)
    assert np.array_equal(eng.detect_stream(both, TAU).cpu().numpy(), np.concatenate([want, want + len(x)]))


# ---- windows that hold whole 2^14-sample segments ---------------------------------------------------------------------
# det_rho_kernel rebuilds the sums of the window in front of a tile from two prefixes that restart every 2^14 samples plus
# the totals of the whole segments in between.  At Lc = 5760 (above) no window holds a whole segment; at the standard's
# N = 4096 every chirp is longer than 2^14 samples.  Two geometries, P = 1, D = 1, two packets and the closing chirp:
#   "c4096": N = 4096, CP = 1184 (the standard's C modes): Lc = 26 400, a window reaches over one or two segment
#            boundaries behind its first: the loop over whole segments runs 0 or 1 times per tile;
#   "n8192": N = 8192, CP = 1024: Lc = 46 080, two or three boundaries, the loop runs 1 or 2 times.
# The tolerance is the file's: 1e-9 on the lags with V >= 1e-6 max V.  Largest |rho_gpu - rho_ref| measured on the MI355X:
# 1.7e-15 (c4096) and 1.4e-15 (n8192) over clean / i16 / u8 / nan, 2.3e-15 over the pieces (DESIGN 3.6 has the table).
# With the loop's additions taken out of a scratch build these cases fail (rho off by 0.62 / 0.85), the ones above pass.
SEG = 1 << 14


class Geo:
    def __init__(self, N, CP):
        K = N // 2 - 1
        known = load("g1_n1024_qpsk")["known_bits"]
        known = np.tile(known, -(-2 * K // len(known)))
        self.p = params_of(load("g1_n1024_qpsk"), N=N, CP=CP, P=1, D=1, lo=1, hi=K, known_bits=known)
        self.Lc, self.frame = self.p.Lc, self.p.frame_len
        self.chirp = orc.chirp_replica(self.p)
        self.lead = 8000
        self.cases, self.engines = {}, {}

    def stream(self, seed=1):
        p, rs = self.p, np.random.RandomState(seed)
        bits = rs.randint(0, 2, 2 * p.D * p.C * p.mu)
        fill = orc.qpsk_table()[0][rs.randint(0, 4, p.K - p.C)]
        x = orc.tx_stream(bits, fill, p, lead=self.lead, tail=8000)
        chirps = self.lead + self.frame * np.arange(3)
        return x, (chirps + self.Lc - 2).astype(np.int64)

    def case(self, name):
        if name not in self.cases:
            x, want = self.stream()
            if name == "awgn":
                x = x + np.random.RandomState(2).normal(0.0, np.sqrt(np.mean(self.chirp ** 2)), len(x))
            elif name == "u8":
                x = np.round(128 + 40 * x).astype(np.uint8)
            elif name == "i16":
                x = np.round(20000 * x).astype(np.int16)
            elif name == "nan":
                x = x.copy()
                x[self.lead + self.frame + self.Lc + 2000] = np.nan       # inside the second packet's body
            q, V = detect_ref.rho(x, self.chirp)
            assert np.array_equal(detect_ref.detect(q, len(x), self.Lc, TAU), want), name
            self.cases[name] = (x, want, q, V)
        return self.cases[name]

    def eng_for(self, x):
        dt = {np.dtype("float64"): torch.float64, np.dtype("float32"): torch.float32, np.dtype("uint8"): torch.uint8,
          np.dtype("int16"): torch.int16}[x.dtype]
        if dt not in self.engines:
            self.engines[dt] = engine_for(self.p, in_dtype=dt)
        return self.engines[dt]


_geos = {}


def geo(name):
    if name not in _geos:
        _geos[name] = Geo(*{"c4096": (4096, 1184), "n8192": (8192, 1024)}[name])
    return _geos[name]


def whole_segments(Lc, n):
    """How many whole segments the window in front of each tile holds (the trip count of the kernel's loop over G1), over the
    tiles of a one-piece call on n samples."""
    t = np.arange((Lc - 1) // 1024, (n - 1) // 1024 + 1)
    jl = t * 1024 - Lc
    return np.where(jl > 0, np.maximum(t // 16 - (jl // 1024) // 16 - 1, 0), t // 16)


@pytest.mark.parametrize("name", ["clean", "i16", "u8", "nan"])
@pytest.mark.parametrize("gname", ["c4096", "n8192"])
def test_rho_and_detections_where_a_window_spans_whole_segments(gname, name):
    G = geo(gname)
    x, want, q, V = G.case(name)
    trips = whole_segments(G.Lc, len(x))
    assert sorted(set(trips.tolist())) == {"c4096": [0, 1], "n8192": [1, 2]}[gname]        # (+ the partly covered one in front)
    assert set(whole_segments(LC, len(case("clean")[0])).tolist()) == {0}                # the geometry above never gets there
    eng = G.eng_for(x)
    peaks, got = eng.detect_stream(x, TAU, want_rho=True)
    got = got.cpu().numpy()
    assert np.array_equal(peaks.cpu().numpy(), want)
    agree(got, q, V, 1e-9, least=G.frame)
    assert np.array_equal(np.isnan(got), np.isnan(q))
    if name == "clean":
        assert np.abs(got[want + 1] - 1.0).max() < 1e-9
    if name == "nan":
        assert np.isnan(got).sum() == G.Lc


@pytest.mark.parametrize("gname", ["c4096", "n8192"])
def test_piece_invariance_where_a_window_spans_whole_segments(gname):
    """Pieces whose buffers end on a multiple of 2^14 samples, inside a segment, and one sample to either side of the boundary;
    every later piece's buffer starts Lc - 1 samples in front of its cut, so its segments lie elsewhere in the stream."""
    G = geo(gname)
    x, want, q, V = G.case("awgn")
    eng = G.eng_for(x)
    n, Lc = len(x), G.Lc
    one = eng.detect_stream(x, TAU, want_rho=True)[1].cpu().numpy()
    on = 4 * SEG                                                  # the first piece ends on a segment boundary ...
    base = on - (Lc - 1)                                          # (where the second piece's buffer starts)
    inside = base + ((Lc - 1) // SEG + 2) * SEG + 5000            # ... the second 5000 samples into a segment of its buffer
    assert on % SEG == 0 and (inside - base) % SEG == 5000 and on < inside < n - Lc
    cuttings = [[0, on, inside, n], [0, on - 1, n], [0, on + 1, n], [0, 3 * SEG, n]]
    for cuts in cuttings:
        found, got = pieces(eng, x, cuts, Lc)
        assert np.array_equal(found, want), cuts
        assert np.abs(got - one).max() <= 2e-9
        agree(got, q, V, 1e-9, least=G.frame)
