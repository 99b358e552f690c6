"""NumPy restatement of the self-normalised chirp detection, independent of the kernels: `rho` from one
zero-padded FFT product and extended-precision running sums, `detect` by looking at every neighbourhood, `segment` by the
spacing of the detections."""
import numpy as np

GUARD = 2.0 ** -36


def rho(r, chirp):
    """-> (rho [n + Lc - 1], V [n + Lc - 1]) at the full-convolution lags g: the Pearson correlation of the window
    r[g - Lc + 1 .. g] with the chirp and the window's centred energy; both 0 on the partial windows (g < Lc - 1, g > n - 1).
    rho = 0 where V <= 2^-36 x the largest V so far (a window of identical samples has V = 0 exactly), NaN where the window
    holds a sample that is not finite (V is NaN there too)."""
    r = np.asarray(r, dtype=np.float64)
    c = np.asarray(chirp, dtype=np.float64)
    n, Lc = len(r), len(c)
    bad = ~np.isfinite(r)
    z = np.where(bad, 0.0, r)
    shift = z[~bad].mean() if (~bad).any() else 0.0             # (rho does not change under a shift)
    z = np.where(bad, 0.0, z - shift).astype(np.longdouble)
    plen = n + Lc - 1
    nfft = 1 << int(np.ceil(np.log2(plen)))
    P = np.fft.irfft(np.fft.rfft(z.astype(np.float64), nfft) * np.fft.rfft(c[::-1], nfft), nfft)[:plen]
    out, V = np.zeros(plen), np.zeros(plen)
    if n < Lc:
        return out, V
    c1 = np.concatenate([[0], np.cumsum(z)])
    c2 = np.concatenate([[0], np.cumsum(z * z)])
    cb = np.concatenate([[0], np.cumsum(bad)])
    step = np.concatenate([[0, 0], np.cumsum(np.diff(r) != 0)])  # step[j] = changes of value among r[0 .. j-1]
    g = np.arange(Lc - 1, n)                                     # window = samples [g - Lc + 1, g + 1)
    S1, S2 = c1[g + 1] - c1[g - Lc + 1], c2[g + 1] - c2[g - Lc + 1]
    v = np.asarray(S2 - S1 * S1 / Lc, dtype=np.float64)
    v[step[g + 1] - step[g - Lc + 2] == 0] = 0.0                 # identical samples: exactly no energy
    holds_bad = cb[g + 1] - cb[g - Lc + 1] > 0
    vrun = np.maximum.accumulate(np.where(holds_bad, 0.0, v))
    Sc, Ec = c.astype(np.longdouble).sum(), (c.astype(np.longdouble) ** 2).sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.asarray((P[g] - S1 * Sc / Lc) / np.sqrt((Ec - Sc * Sc / Lc) * v.astype(np.longdouble)), dtype=np.float64)
    q[v <= GUARD * vrun] = 0.0
    q[holds_bad] = np.nan
    v[holds_bad] = np.nan
    out[g], V[g] = q, v
    return out, V


def detect(rho_all, n, Lc, tau):
    """-> detections g - 1 (ascending): the full-window lags g with rho[g] > tau and rho[g] the largest over the full-window
    lags in (g - Lc, g + Lc), the smallest lag winning a tie.  A rho that is not finite is no candidate."""
    q = np.where(np.isfinite(rho_all), rho_all, -np.inf)
    lo, hi = Lc - 1, n - 1
    found = []
    for g in np.flatnonzero(q > tau):
        if not lo <= g <= hi:
            continue
        a, b = max(lo, g - Lc + 1), min(hi, g + Lc - 1)
        w = q[a: b + 1]
        if q[g] == w.max() and a + int(np.argmax(w)) == g:
            found.append(g - 1)
    return np.array(found, dtype=np.int64)


def segment(detections, frame_len, max_gap, slack=0):
    """All detections of a finished stream -> the transmissions, each the array of its detections: two neighbours belong
    to one transmission iff their spacing lies in [frame_len - slack, frame_len + max_gap]."""
    d = np.asarray(detections, dtype=np.int64)
    if len(d) == 0:
        return []
    gap = np.diff(d)
    cut = np.flatnonzero((gap < frame_len - slack) | (gap > frame_len + max_gap)) + 1
    return [part for part in np.split(d, cut)]
