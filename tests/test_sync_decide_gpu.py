"""gf3_sync_decide on planted kept-lag lists: the peak rule on raw triples (division by the maximum first, extremum test,
threshold), the compaction of the survivors across ck_decide_kernel's 1024-wide steps, and the suppression walk -- against
a NumPy restatement of chirp_method's rule (OFDM.py:359-370) written here."""
import ctypes as C

import numpy as np
import pytest
import torch

from gf3_audio_modem_amd import _lib
from gf3_audio_modem_amd._lib import Gf3Error
from tests.util import engine_for, load, params_of

pytestmark = pytest.mark.gpu

STEP = 1024                                                  # ck_decide_kernel looks at this many listed lags per step


@pytest.fixture(scope="module")
def eng():
    return engine_for(params_of(load("g1_n1024_qpsk")))       # N = 1024


def restate(idx, val3, mx, thresh, Lc, nz_total):
    """-> (candidates, peaks): p = P / max first, then (p1 - p0)(p2 - p1) <= 0 and p1 > thresh; the walk of
    oracle.pick_peaks over the ascending candidates, the wipe of the except-branch included."""
    with np.errstate(invalid="ignore"):
        p = val3 / mx
        cand = idx[((p[:, 1] - p[:, 0]) * (p[:, 2] - p[:, 1]) <= 0) & (p[:, 1] > thresh)]
    peaks, last = [], None
    for i in cand:
        if last is not None and i <= last + Lc:
            continue
        if i + Lc >= nz_total:
            return cand, np.zeros(0, np.int64)
        peaks.append(i)
        last = i
    return cand, np.array(peaks, np.int64)


def planted(n, mx, thresh, Lc, spacing, seed):
    """n triples, about half of which pass the rule, in every way a triple can pass or fail; the ones around every step
    boundary pass.  Multiples of the maximum by binary fractions, so that p1 == thresh exactly where that is meant.
    spacing "wide": every candidate is more than Lc after the one before (the peaks are the candidates, so the
    compaction is seen entry by entry); "dense": most candidates fall to the suppression."""
    rs = np.random.RandomState(seed)
    kinds = np.array([[0.25, 0.875, 0.5],                    # pass: a maximum above the threshold
                      [0.875, 0.625, 0.75],                  # pass: a minimum above the threshold
                      [0.75, 0.75, 0.75],                    # pass: a flat run (the product is 0)
                      [0.5, 0.75, 0.75],                     # pass: a flat step
                      [0.5, 0.625, 0.75],                    # fail: monotone
                      [0.125, 0.25, 0.125],                  # fail: a maximum below the threshold
                      [0.25, thresh, 0.25],                  # fail: p1 == thresh, the comparison is strict
                      [0.25, np.nan, 0.5]])                  # fail: NaN compares false
    k = rs.randint(0, len(kinds), n)
    for b in range(STEP, n + 2, STEP):                       # survivors on both sides of every step boundary
        k[max(b - 2, 0): min(b + 2, n)] = rs.randint(0, 4, min(b + 2, n) - max(b - 2, 0))
    val3 = kinds[k] * mx
    gaps = rs.randint(Lc + 1, Lc + 40, n) if spacing == "wide" else rs.randint(1, Lc // 2, n)
    return 10 + np.cumsum(gaps).astype(np.int64), val3


def decide(eng, idx, val3, mx, nz_total, cap):
    n = len(idx)
    dev = eng.device
    d_idx = torch.from_numpy(idx).to(dev) if n else None
    d_val = torch.from_numpy(np.ascontiguousarray(val3)).to(dev) if n else None
    d_max = torch.tensor([mx], dtype=torch.float64, device=dev)
    peaks = torch.full((cap,), -1, dtype=torch.int64, device=dev)
    work = torch.zeros((int(eng.lib.gf3_sync_decide_workspace_bytes(eng._h, n)),), dtype=torch.uint8, device=dev)
    cnt = C.c_int64(-1)
    eng._check(eng.lib.gf3_sync_decide(eng._h, _lib.ptr(d_idx), _lib.ptr(d_val), n, _lib.ptr(d_max), int(nz_total), _lib.ptr(peaks),
                                       cap, C.byref(cnt), _lib.ptr(work), eng._stream()))
    return peaks[: cnt.value].cpu().numpy()


@pytest.mark.parametrize("spacing", ["wide", "dense"])
@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2085])
def test_decide_compacts_across_steps(eng, n, spacing):
    Lc, thresh, mx = eng.cfg.chirp_length, eng.cfg.thresh, 4.0
    idx, val3 = planted(n, mx, thresh, Lc, spacing, seed=n + (spacing == "dense"))
    far = int(idx[-1]) + Lc + 1 if n else 100                # no candidate reaches the end of the stream
    cand, want = restate(idx, val3, mx, thresh, Lc, far)
    if n > 1:
        assert 0.35 * n <= len(cand) <= 0.65 * n             # about half pass
        for b in range(STEP, n, STEP):
            assert idx[b - 1] in cand and idx[b] in cand     # survivors straddle the boundary
    if spacing == "wide":
        assert np.array_equal(want, cand)
    elif n > 1:
        assert 0 < len(want) < len(cand)
    got = decide(eng, idx, val3, mx, far, cap=n + 4)
    assert np.array_equal(got, want)
    if len(want):
        # the except-branch: the last accepted candidate within Lc of the end wipes everything -- one lag more and it does not
        last = int(want[-1])
        assert len(restate(idx, val3, mx, thresh, Lc, last + Lc)[1]) == 0
        assert len(decide(eng, idx, val3, mx, last + Lc, cap=n + 4)) == 0
        assert np.array_equal(decide(eng, idx, val3, mx, last + Lc + 1, cap=n + 4), restate(idx, val3, mx, thresh, Lc, last + Lc + 1)[1])


def test_decide_negative_maximum(eng):
    """The division is by the SIGNED maximum: with a negative one the order turns round, and only negative values can
    pass the threshold."""
    Lc, thresh = eng.cfg.chirp_length, eng.cfg.thresh
    idx, val3 = planted(1500, 4.0, thresh, Lc, "wide", seed=3)
    val3[::3] *= -1.0
    far = int(idx[-1]) + Lc + 1
    cand, want = restate(idx, val3, -4.0, thresh, Lc, far)
    assert 100 < len(want) < 500 and np.all(val3[np.isin(idx, want), 1] < 0)
    assert np.array_equal(decide(eng, idx, val3, -4.0, far, cap=1504), want)


def test_decide_nan_maximum_gives_no_peaks(eng):
    Lc, thresh = eng.cfg.chirp_length, eng.cfg.thresh
    idx, val3 = planted(1500, 4.0, thresh, Lc, "wide", seed=4)
    far = int(idx[-1]) + Lc + 1
    assert len(restate(idx, val3, np.nan, thresh, Lc, far)[1]) == 0
    assert len(decide(eng, idx, val3, float("nan"), far, cap=1504)) == 0


def test_decide_capacity_one_short(eng):
    Lc, thresh = eng.cfg.chirp_length, eng.cfg.thresh
    idx, val3 = planted(1500, 4.0, thresh, Lc, "wide", seed=5)
    far = int(idx[-1]) + Lc + 1
    want = restate(idx, val3, 4.0, thresh, Lc, far)[1]
    assert np.array_equal(decide(eng, idx, val3, 4.0, far, cap=len(want)), want)       # exactly full
    with pytest.raises(Gf3Error, match=f"gf3_sync_decide: {len(want)} peaks exceed capacity {len(want) - 1}"):
        decide(eng, idx, val3, 4.0, far, cap=len(want) - 1)
