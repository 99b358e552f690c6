"""NumPy restatement (float64) of adaptive bit loading, written from the definitions, not from the kernels,
on tests/noise_ref.py's `maxlog`, `decide` and `weights`:

  order[c] in {0, 2, 4, 6};  Bs = sum(order);  off[c] = sum(order[:c]);  bits travel packet -> symbol -> carrier -> bit
  carrier of order m > 0: the Gray-coded square 2^m-QAM of unit energy (`table`); order 0: the bin's pilot symbol
  v[f, c]   = (1/D) sum_l |eq[f, l, c] - s|^2, s the carrier's own table's decision; the pilot symbol at order 0
  LLR[f, l, off[c] + b] = (float32)(maxlog(eq[f, l, c]; table(order[c]))[b] * w), +0 where w = 0
  w = noise_ref.weights(v)[f, c]  |  (|Hs| + (|He| - |Hs|) (l + P/2) / (D + P))^2 at the carrier's bin  |  1

eq is [F*D, C] (packet -> symbol -> carrier)."""
import functools

import numpy as np

from tests import noise_ref as NR


@functools.lru_cache(maxsize=None)
def table(m):
    """(points, bits) of the square 2^m-QAM: axis level i = (2i - (L-1)) / sqrt(2 (L^2 - 1) / 3) carries the Gray label
    i ^ (i >> 1); label bits MSB first, the first m/2 on the I axis."""
    h = m // 2
    L = 1 << h
    lv = {i ^ (i >> 1): (2 * i - (L - 1)) / np.sqrt(2.0 * (L * L - 1) / 3.0) for i in range(L)}
    labels = np.arange(1 << m)
    pts = np.array([complex(lv[lab >> h], lv[lab & (L - 1)]) for lab in labels])
    return pts, ((labels[:, None] >> np.arange(m - 1, -1, -1)) & 1).astype(np.int64)


def layout(order):
    off = np.concatenate([[0], np.cumsum(np.asarray(order, dtype=np.int64))])
    return int(off[-1]), off


def map_loaded(bits, order, known):
    """bits [n_sym * Bs] -> complex [n_sym, C]; known [C]: the pilot symbol of each carrier's bin."""
    order = np.asarray(order)
    Bs, off = layout(order)
    rows = np.asarray(bits, dtype=np.int64).reshape(-1, Bs)
    out = np.empty((len(rows), len(order)), dtype=np.complex128)
    for c, m in enumerate(order.tolist()):
        if m == 0:
            out[:, c] = known[c]
        else:
            lab = (rows[:, off[c]: off[c] + m] << np.arange(m - 1, -1, -1)).sum(axis=1)
            out[:, c] = table(m)[0][lab]                   # (the table is in ascending label order)
    return out


def noise_estimate(eq, order, known, D):
    eq = np.asarray(eq, dtype=np.complex128)
    order = np.asarray(order)
    v = np.empty((eq.shape[0] // D, eq.shape[1]))
    for m in np.unique(order):
        cs = np.flatnonzero(order == m)
        if m == 0:
            with np.errstate(invalid="ignore", over="ignore"):
                e = eq[:, cs] - np.asarray(known)[cs]
                v[:, cs] = (e.real ** 2 + e.imag ** 2).reshape(-1, D, len(cs)).sum(axis=1) / D
        else:
            v[:, cs] = NR.noise_estimate(eq[:, cs], table(int(m))[0], D)
    return v


def csi_weights(Hs, He, bins, P, D):
    """[F, D, C]: the reference's magnitude model, squared, at each carrier's (1-based) bin."""
    s = np.abs(np.asarray(Hs))[:, None, np.asarray(bins) - 1]
    e = np.abs(np.asarray(He))[:, None, np.asarray(bins) - 1]
    l = np.arange(D)[None, :, None]
    return (s + (e - s) * (l + P / 2.0) / (D + P)) ** 2


def soft_demap(eq, order, D, w=None):
    """-> float32 [F*D*Bs].  w: None (unit), [F, C] (per carrier) or [F, D, C]."""
    eq = np.asarray(eq, dtype=np.complex128)
    order = np.asarray(order)
    Bs, off = layout(order)
    n, C = eq.shape
    if w is None:
        w = np.ones((n // D, 1, C))
    w = np.asarray(w, dtype=np.float64)
    if w.ndim == 2:
        w = w[:, None, :]
    w = np.broadcast_to(w, (n // D, D, C)).reshape(n, C)
    out = np.zeros((n, Bs), dtype=np.float32)
    for m in (2, 4, 6):
        pts, bits = table(m)
        for c in np.flatnonzero(order == m):
            with np.errstate(invalid="ignore", over="ignore"):
                llr = NR.maxlog(eq[:, c], pts, bits) * w[:, c, None]
            out[:, off[c]: off[c] + m] = np.where(w[:, c, None] == 0, 0.0, llr).astype(np.float32)
    return out.reshape(-1)


def soft_demap_nw(eq, var, order, D):
    return soft_demap(eq, order, D, NR.weights(var))


def soft_demap_csi(eq, Hs, He, bins, order, P, D):
    return soft_demap(eq, order, D, csi_weights(Hs, He, bins, P, D))


def hard_bits(llr):
    return (np.asarray(llr) < 0).astype(np.int64)
