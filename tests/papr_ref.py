"""Tone reservation on the filler carriers, restated in NumPy: what gf3_tone_reserve (csrc/gf3rx_papr.hip) computes per
data symbol.  Test reference only.

Per data symbol: X_k are the values tx_frames sends on the data carriers; the reserved set is carriers 1 .. K that are
not data carriers, ascending, Ku = K - C of them; x(R) is the real N-sample symbol of the Hermitian spectrum with X on
the data bins, R on the reserved bins and DC and Nyquist zero, in np.fft.ifft scaling (without the frame's x2).

    sigma = sqrt(2 sum |X_k|^2) / N        the rms of the data alone
    A = sigma 10^(target_db / 20)          the clip level
    L = 10^(tone_limit_db / 20)            the largest |tone|

    R = 0, best = (max |x(R)|, R, 0)
    for i = 1 .. I:
        c = x(R) - clip(x(R), -A, A);  stop if c is zero everywhere
        R <- R - N / (2 Ku) fft(c) on the reserved bins
        every |R_k| > L is scaled back to L
        max |x(R)| strictly below the best peak: this iterate is the best (the first minimum wins)

Iterate 0 -- zero tones -- takes part, so the result is never worse than a zero filler."""
import numpy as np

from oracle import gf3_oracle as orc


def reserved_bins(p):
    """Carriers 1 .. K outside the data carriers, ascending (1-based FFT bins)."""
    return np.delete(np.arange(1, p.K + 1), np.asarray(p.data_carriers) - 1)


def symbol(X, R, p, rsv=None):
    """x(R): [N] real samples of one symbol, data values X [C] in data_carriers order, tones R [Ku]."""
    half = np.zeros(p.N // 2 + 1, dtype=complex)
    half[np.asarray(p.data_carriers)] = X
    half[reserved_bins(p) if rsv is None else rsv] = R
    return np.fft.irfft(half, p.N)                                   # == np.fft.ifft of the Hermitian N-bin row, real part


def reserve_symbol(X, p, target_db=6.0, tone_limit_db=6.0, iterations=16):
    """-> (best tones [Ku], report row (peak at R = 0, best peak, best index, rms of the best symbol), peaks of every
    iterate that was formed)."""
    rsv = reserved_bins(p)
    Ku = len(rsv)
    sigma = np.sqrt(2.0 * np.sum(np.abs(X) ** 2)) / p.N
    A = sigma * 10.0 ** (target_db / 20.0)
    L = 10.0 ** (tone_limit_db / 20.0)
    R = np.zeros(Ku, dtype=complex)
    x = symbol(X, R, p, rsv)
    peaks = [float(np.abs(x).max())]
    best_R, best_i, best_x = R, 0, x
    for i in range(1, iterations + 1):
        c = x - np.clip(x, -A, A)
        if not c.any():
            break
        R = R - (p.N / (2.0 * Ku)) * np.fft.fft(c)[rsv]
        mag = np.abs(R)
        over = mag > L
        R[over] = R[over] * (L / mag[over])
        x = symbol(X, R, p, rsv)
        peaks.append(float(np.abs(x).max()))
        if peaks[-1] < peaks[best_i]:
            best_R, best_i, best_x = R, i, x
    row = np.array([peaks[0], peaks[best_i], float(best_i), float(np.sqrt(np.mean(best_x ** 2)))])
    return best_R, row, np.array(peaks)


def tone_reserve(bits, p, target_db=6.0, tone_limit_db=6.0, iterations=16):
    """Engine.tone_reserve on payload bits (F D C mu of them): -> (tones [F, D, Ku], report [F, D, 4], peaks: list of the
    iterate peaks per symbol)."""
    X = orc.map_bits(np.asarray(bits).reshape(-1, p.C, p.mu), p)
    got = [reserve_symbol(row, p, target_db, tone_limit_db, iterations) for row in X]
    Ku = p.K - p.C
    return (np.array([g[0] for g in got]).reshape(-1, p.D, Ku), np.array([g[1] for g in got]).reshape(-1, p.D, 4),
            [g[2] for g in got])


def near_tie(peaks, rel=1e-9):
    """Whether the two smallest iterate peaks of a symbol lie within `rel` of each other: rounding may then pick either."""
    if len(peaks) < 2:
        return False
    a, b = np.sort(peaks)[:2]
    return bool(b - a <= rel * b)
