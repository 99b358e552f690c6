"""NumPy restatement of the receive windowing ahead of the demodulator (gf3_window_frames), written from its definition, and
the interferer scenario the CPU and the GPU test share.

Packet f: body [s_f, s_f + M S), M = 2P + D, S = N + CP.  Symbol m with samples s[0 .. S), ramp r[0 .. L), 1 <= L <= CP:

    out[S - L + i] = s[S - L + i] (1 - r[i]) + s[CP - L + i] r[i]          (i = 0 .. L - 1)

every other sample copied; the rows are packed [F, M S] in the storage type (fp64 as is, float32 by a cast, int16 / uint8 by
rint, half to even, clamped).  report[f, m] = (sum_i (s[S-L+i] - s[CP-L+i])^2, sum_i (s[S-L+i]^2 + s[CP-L+i]^2)), both NaN where one of
those 2L samples is not finite.  A body that is not inside the samples: status 1, a row of zeros, a NaN report.

`work` is the type the arithmetic runs in: float64 restates the kernel, np.longdouble gives a reference whose own rounding
(2^-64 on x86) is far below the kernel's, so that a tolerance counted in fp64 roundings of the kernel alone holds."""
import numpy as np

from oracle import gf3_oracle as orc
from tests.resample_ref import to_storage                   # the storage rule the two stages share


def ramp(L):
    """The raised cosine the Engine passes: r[i] = 0.5 - 0.5 cos(pi (i + 0.5) / L); r[i] + r[L - 1 - i] = 1."""
    return 0.5 - 0.5 * np.cos(np.pi * (np.arange(L, dtype=np.float64) + 0.5) / L)


def status_of(starts, n_body, n_in):
    return np.array([1 if (s < 0 or n_body > n_in or s > n_in - n_body) else 0 for s in starts], dtype=np.int32)


def window_symbols(sym, N, CP, L, r=None, work=np.float64):
    """sym [..., S] in any type -> (the windowed symbols in `work`, before the storage rounding, report [..., 2] in `work`)"""
    r = (ramp(L) if r is None else np.asarray(r)).astype(work)
    s = np.asarray(sym).astype(work)
    S = N + CP
    a, b = s[..., S - L:], s[..., CP - L: CP]
    out = s.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        out[..., S - L:] = a * (1 - r) + b * r
        rep = np.stack([((a - b) ** 2).sum(axis=-1), (a * a + b * b).sum(axis=-1)], axis=-1)
    bad = ~(np.isfinite(a).all(axis=-1) & np.isfinite(b).all(axis=-1))
    rep[bad] = np.nan
    return out, rep


def window_rows(x, starts, N, CP, M, L, r=None, work=np.float64):
    """-> (rows [F, M S] in x's dtype, the same before the storage rounding (`work`), status int32 [F], report [F, M, 2])"""
    x = np.asarray(x)
    S = N + CP
    n_body = M * S
    starts = np.asarray(starts, dtype=np.int64)
    status = status_of(starts, n_body, len(x))
    raw = np.zeros((len(starts), n_body), dtype=work)
    report = np.full((len(starts), M, 2), np.nan, dtype=work)
    for f, s in enumerate(starts):
        if status[f]:
            continue
        out, report[f] = window_symbols(x[s: s + n_body].reshape(M, S), N, CP, L, r, work)
        raw[f] = out.reshape(-1)
    return to_storage(raw, x.dtype), raw, status, report


def mismatch_db(report):
    """report [..., M, 2] -> 10 log10 of sum_m report[.., 0] / sum_m report[.., 1] per packet: `last_window_report`'s figure"""
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.asarray(report, dtype=np.float64).sum(axis=-2)
        return 10.0 * np.log10(s[..., 0] / s[..., 1])


# ---- the interferer scenario -----------------------------------------------------------------------------------------------
TAPS, SNR_DB, TONE_HZ, FS, TAPER = 40, 25.0, 9005.3, 48000.0, 128
LEAD, TAIL = 300, 400


def channel(seed=5):
    """A channel of 40 taps: a direct path of 1 and a seeded tail that decays by 1 / e every 8 samples."""
    rng = np.random.default_rng(seed)
    h = rng.normal(size=TAPS) * np.exp(-np.arange(TAPS) / 8.0) * 0.5
    h[0] = 1.0
    return h


def body_rms(clean, p, n_packets=1):
    """RMS of the recording over the packets' bodies (a stream of tx_stream with lead = LEAD and no gaps)"""
    at = LEAD + p.Lc
    return float(np.sqrt(np.mean(clean[at: at + n_packets * p.frame_len - p.Lc] ** 2)))


def interfered(clean, rms, level_db, seed=5):
    """clean + white noise SNR_DB below `rms` (seeded) + one tone at TONE_HZ, off the carrier grid, whose power lies level_db
    above rms^2 (None: no tone)"""
    n = len(clean)
    out = clean + rms * 10.0 ** (-SNR_DB / 20.0) * np.random.default_rng(seed).normal(size=n)
    if level_db is not None:
        amp = rms * np.sqrt(2.0) * 10.0 ** (level_db / 20.0)
        out = out + amp * np.sin(2.0 * np.pi * TONE_HZ / FS * np.arange(n) + 0.7)
    return out


def receive(r, p, L=0):
    """The oracle's receive with the restated stage between its sync and its demodulator -> orc.demod_frames' outputs"""
    starts = orc.frame_starts(orc.chirp_method(r, p))
    if L:
        rows, _, status, report = window_rows(r, starts, p.N, p.CP, p.M, L)
        assert not status.any()
        o = orc.demod_frames(rows.reshape(-1), np.arange(len(starts)) * p.M * p.S, p)
        o["report"] = report
    else:
        o = orc.demod_frames(r, starts, p)
    o["starts"] = starts
    return o


def sinr_db(eq, sent):
    """Per-carrier SINR of the equalised symbols eq [F D, C] against the points sent, in dB [C]"""
    err = np.mean(np.abs(eq - sent) ** 2, axis=0)
    return 10.0 * np.log10(np.mean(np.abs(sent) ** 2, axis=0) / err)
