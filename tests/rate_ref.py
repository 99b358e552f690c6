"""NumPy restatement of the whole-stream rate conversion (gf3_resample_stream, include/gf3rx.h): the rule with its index
arithmetic written as the header states it, on the table of tests/resample_ref.py; the output counts by brute force; and
`recording`, an exact synthesiser of a transmission as a sound card at another rate records it, which uses none of the
code under test."""
import math

import numpy as np

from oracle import gf3_oracle as orc
from tests import resample_ref as RR

L = RR.L
RATIOS = [147 / 160, 160 / 147, 2.0, 0.5, 4.0, 0.25, 44100.7 / 48000]


def reach(r, T):
    """Tw: input samples to either side of floor(t_j) that output j reads (T where r <= 1, ceil(T r) where r > 1)."""
    return int(math.ceil(T * r)) if r > 1.0 else T


def coefficients(j, r, T):
    """Outputs j (int64 array) -> (i int64 [n]: floor(t_j), d int64 [W]: the taps' distances from i, c float64 [n, W])."""
    h = RR.table(T)
    t = np.asarray(j, dtype=np.int64).astype(np.float64) * r                 # one rounding
    i = np.floor(t)
    mu = t - i
    if r <= 1.0:                                                            # resample_ref.resample_rows' rule
        q = mu * L
        p = np.minimum(q.astype(np.int64), L - 1)
        a = q - p
        c = h[p] + a[:, None] * (h[p + 1] - h[p])
        d = np.arange(2 * T) - T + 1
        return i.astype(np.int64), d, c
    rho = 1.0 / r
    Tw = int(math.ceil(T * r))
    d = np.arange(2 * Tw) - Tw + 1
    v = (d[None, :].astype(np.float64) - mu[:, None]) * rho
    n = np.ceil(v)
    f = n - v
    q = f * L
    p = np.minimum(q.astype(np.int64), L - 1)
    a = q - p
    col = n.astype(np.int64) + T - 1
    inside = (col >= 0) & (col < 2 * T)
    cc = np.clip(col, 0, 2 * T - 1)
    h0, h1 = h[p, cc], h[p + 1, cc]
    c = np.where(inside, rho * (h0 + a * (h1 - h0)), 0.0)
    return i.astype(np.int64), d, c


def whole_count(n_in, r):
    """Outputs of a whole recording of n_in samples: the j >= 0 with (double)j r <= n_in - 1, by brute force."""
    j = np.arange(int((n_in + 2) / r) + 4, dtype=np.int64)
    return int(np.count_nonzero(j.astype(np.float64) * r <= n_in - 1))


def final_count(n_seen, r, T):
    """Outputs that are final after n_seen input samples: floor((double)j r) + Tw <= n_seen - 1, by brute force."""
    j = np.arange(int((n_seen + 2) / r) + 4, dtype=np.int64)
    return int(np.count_nonzero(np.floor(j.astype(np.float64) * r) + reach(r, T) <= n_seen - 1))


def convert(x, r, T, in_origin=0, j0=0, n_out=None):
    """x holds samples in_origin .. in_origin + len(x) - 1 of the stream -> (raw float64 [n_out]: outputs j0 .. j0 + n_out - 1
    before any storage rounding, sum_k |c_k| of every output [n_out]).  Samples outside x read as 0; ascending k."""
    x64 = np.asarray(x).astype(np.float64)
    n_in = len(x64)
    if n_out is None:
        n_out = max(whole_count(in_origin + n_in, r) - j0, 0)
    i, d, c = coefficients(np.arange(j0, j0 + n_out, dtype=np.int64), r, T)
    idx = i[:, None] + d[None, :] - in_origin
    ok = (idx >= 0) & (idx < n_in)
    xs = np.where(ok, x64[np.clip(idx, 0, max(n_in - 1, 0))], 0.0) if n_in else np.zeros(idx.shape)
    acc = np.zeros(n_out)
    for k in range(len(d)):                                                 # ascending k
        acc = acc + c[:, k] * xs[:, k]
    return acc, np.abs(c).sum(axis=1)


def convert_blocks(x, r, T, sizes):
    """The stream x fed in blocks of `sizes` samples (the last size repeats), each block converted as far as its outputs
    are final with the tail the next outputs still read carried over, the rest at the end -> raw float64, as `convert`."""
    out, held, origin, seen, done, at = [], np.zeros(0), 0, 0, 0, 0
    sizes = list(sizes)
    while seen < len(x):
        size = sizes[min(at, len(sizes) - 1)]
        at += 1
        block = np.asarray(x[seen: seen + size], dtype=np.float64)
        held = np.concatenate([held, block])
        seen += len(block)
        upto = final_count(seen, r, T)
        if upto > done:
            out.append(convert(held, r, T, in_origin=origin, j0=done, n_out=upto - done)[0])
            done = upto
        keep = max(int(math.floor(float(done) * r)) - reach(r, T) + 1, origin)      # the first sample output `done` reads
        held, origin = held[keep - origin:], keep
    total = whole_count(len(x), r)
    out.append(convert(held, r, T, in_origin=origin, j0=done, n_out=total - done)[0])
    return np.concatenate(out)


# ---- a transmission as a sound card at another rate records it --------------------------------------------------------
def recording(bits, fill_syms, p, rate, lead=0, tail=2, eps_extra=0.0):
    """orc.tx_stream(bits, fill_syms, p, lead=lead, tail=tail) as a recorder running at `rate` samples per second takes it:
    sample j at the transmitter's time j (1 + eps), eps = (p.fs / rate)(1 + eps_extra) - 1 (eps_extra: a clock offset on top
    of the nominal rate, in the convention of resample_ref.drifted_stream), behind an ideal anti-alias filter: every
    symbol's spectrum is zeroed from the recording's Nyquist frequency on.  Built like drifted_stream from
    resample_ref._trig; the chirps (0 .. p.f1, below every Nyquist frequency used) from their closed form."""
    rows = orc.tx_frames(bits, fill_syms, p)
    F = rows.shape[0]
    step = (p.fs / rate) * (1.0 + eps_extra)
    total = lead + F * p.frame_len + p.Lc + tail
    n = int(np.floor((total - 1) / step)) + 1
    tau = np.arange(n) * step
    out = np.zeros(n)
    Lc = p.Lc
    t1 = Lc / p.fs
    cstep = t1 / (Lc - 1)
    beta = (p.f1 - p.f0) / t1
    cut = int(math.ceil(p.N * (rate / 2.0) / p.fs))                          # the first bin at or above the recorder's Nyquist

    def span(a, b):
        return np.searchsorted(tau, a, "left"), np.searchsorted(tau, b, "left")

    def chirp_at(a):
        lo, hi = span(a, a + Lc)
        t = (tau[lo:hi] - a) * cstep
        out[lo:hi] = np.cos(2 * np.pi * (p.f0 * t + 0.5 * beta * t * t)) / 5

    for f in range(F):
        a = lead + f * p.frame_len
        chirp_at(a)
        for m in range(p.M):
            b = a + Lc + m * p.S
            lo, hi = span(b, b + p.S)
            if hi > lo:
                X = np.fft.rfft(rows[f, Lc + m * p.S + p.CP: Lc + (m + 1) * p.S])
                X[cut:] = 0.0
                out[lo:hi] = RR._trig(X, tau[lo] - (b + p.CP), step, hi - lo)
    chirp_at(lead + F * p.frame_len)
    return out
