"""NumPy restatement of the sampling-clock correction (csrc/gf3rx_resample.hip, include/gf3rx.h): the coefficient table,
the resampler with the index arithmetic written as the header states it, the storage rounding, the status rule and the
offset a fitted slope stands for -- and `drifted_stream`, an exact synthesiser of a stream recorded with a clock offset that
uses none of the code under test."""
import numpy as np

from oracle import gf3_oracle as orc

L = 1024                    # phases of the table (rows 0 .. L)
BETA = 10.0                 # Kaiser window
MAX_EPS = 2e-3              # beyond it (or not finite) a row is copied and status bit 1 set
_TABLES = {}


def table(T):
    """h [L + 1, 2T]: h[p][k] = sinc(u) I0(beta sqrt(1 - (u / T)^2)) / I0(beta), u = (k - T + 1) - p / L, window 0 for
    |u| >= T; sin(pi u) as -(-1)^(k - T + 1) sin(pi p / L), rows 0 and L unit impulses exactly."""
    if T not in _TABLES:
        n = (np.arange(2 * T) - T + 1)[None, :]
        ph = (np.arange(L + 1) / L)[:, None]
        u = n - ph
        sn = np.where(n % 2 != 0, 1.0, -1.0) * np.sin(np.pi * ph)
        inside = np.abs(u) < T
        z = np.where(inside, u / T, 0.0)
        win = np.where(inside, np.i0(BETA * np.sqrt(1.0 - z * z)) / np.i0(BETA), 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            h = sn / (np.pi * u) * win
        h[0] = (n[0] == 0)
        h[L] = (n[0] == 1)
        h.setflags(write=False)
        _TABLES[T] = h
    return _TABLES[T]


def to_storage(v, dtype):
    """fp64 values in a storage type: as they are, a cast for float32, rint (half to even) and a clamp for int16 / uint8."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return np.asarray(v).astype(dtype)
    info = np.iinfo(dtype)
    return np.clip(np.rint(v), info.min, info.max).astype(dtype)


def status_of(starts, eps, n_body, n_in):
    """int32 [F]: bit 0 the body is not inside [0, n_in); bit 1 eps is not finite or |eps| > 2e-3."""
    out = np.zeros(len(starts), dtype=np.int32)
    for f, (s, e) in enumerate(zip(starts, eps)):
        ragged = s < 0 or n_body > n_in or s > n_in - n_body
        bad = not (abs(e) <= MAX_EPS)
        out[f] = (1 if ragged else 0) | (2 if bad else 0)
    return out


def resample_rows(x, starts, n_body, eps, T):
    """-> (rows [F, n_body] in x's dtype, the same before the storage rounding (float64), status int32 [F])"""
    x = np.asarray(x)
    x64 = x.astype(np.float64)
    n_in = len(x)
    starts = np.asarray(starts, dtype=np.int64)
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float64), starts.shape)
    status = status_of(starts, eps, n_body, n_in)
    h = table(T)
    raw = np.zeros((len(starts), n_body))
    taps = np.arange(2 * T)
    for f, s in enumerate(starts):
        if status[f] & 1:
            continue
        e = 0.0 if status[f] & 2 else float(eps[f])
        r = 1.0 / (1.0 + e)
        t = np.arange(n_body).astype(np.float64) * r
        i = np.floor(t)
        mu = t - i
        q = mu * L
        p = np.minimum(q.astype(np.int64), L - 1)
        a = q - p
        c = h[p] + a[:, None] * (h[p + 1] - h[p])
        idx = s + i.astype(np.int64)[:, None] + taps[None, :] - T + 1
        ok = (idx >= 0) & (idx < n_in)
        xs = np.where(ok, x64[np.clip(idx, 0, max(n_in - 1, 0))], 0.0)
        acc = np.zeros(n_body)
        for k in range(2 * T):                                  # ascending k
            acc = acc + c[:, k] * xs[:, k]
        raw[f] = acc
    return to_storage(raw, x.dtype), raw, status


def clock_offset(slope, p):
    """eps = slope N / (2 pi (P + D) S): the slope is the phase per carrier index accrued between the pilot blocks' centres."""
    return np.asarray(slope, dtype=np.float64) * (p.N / (2.0 * np.pi * (p.P + p.D) * p.S))


# ---- an exactly synthesised clock offset ----------------------------------------------------------------------------
def _trig(X, tau0, step, n):
    """The real trigonometric polynomial with rfft spectrum X (N / 2 + 1 bins) at the times tau0 + j step, j = 0 .. n - 1,
    in blocks of 64 times: exp(i w (tau0 + (64 b + c) step)) = exp(i w tau0) exp(i w 64 b step) exp(i w c step)."""
    nb = len(X)
    N = 2 * (nb - 1)
    w = 2.0 * np.pi * np.arange(nb) / N
    weight = np.full(nb, 2.0)
    weight[0] = weight[-1] = 1.0
    B = 64
    blocks = -(-n // B)
    A = X * weight / N * np.exp(1j * w * tau0)
    outer = A[None, :] * np.exp(1j * np.outer(np.arange(blocks) * (B * step), w))
    inner = np.exp(1j * np.outer(w, np.arange(B) * step))
    # (the real part of the product, as two real matrix products)
    return (outer.real @ inner.real - outer.imag @ inner.imag).reshape(-1)[:n]


def drifted_stream(bits, fill_syms, p, eps, lead=0, tail=2, t0=0.0):
    """orc.tx_stream(bits, fill_syms, p, lead=lead, tail=tail) as a receiver records it whose sample j is taken at the
    transmitter's time j (1 + eps) + t0: every symbol's spectrum (an rfft of its body) evaluated as a trigonometric
    polynomial at those times, in the symbol each time falls into (the cyclic prefix is the polynomial's own period); the
    chirps from their closed form; zeros elsewhere.  As many samples as fall inside the transmitted stream."""
    rows = orc.tx_frames(bits, fill_syms, p)
    F = rows.shape[0]
    total = lead + F * p.frame_len + p.Lc + tail
    n = int(np.floor((total - 1 - t0) / (1.0 + eps))) + 1
    tau = np.arange(n) * (1.0 + eps) + t0
    out = np.zeros(n)
    Lc = p.Lc
    t1 = Lc / p.fs
    cstep = t1 / (Lc - 1)
    beta = (p.f1 - p.f0) / t1

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
                out[lo:hi] = _trig(X, tau[lo] - (b + p.CP), 1.0 + eps, hi - lo)
    chirp_at(lead + F * p.frame_len)
    return out
