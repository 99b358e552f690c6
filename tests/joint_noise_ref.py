"""NumPy restatement of the two-speaker receive paths under coloured noise ("Coloured noise on the two-speaker
paths"; include/gf3rx.h), written from the definition on top of the oracle and of tests/mimo_ref.py, tests/stbc_ref.py and
tests/diversity_ref.py, not from the kernels -- TEST INFRASTRUCTURE.

  pilot_noise(x, starts, H, p)           -> v [F, 2 sides, K], status [F]: what the two covers leave of the pilots,
                                            v = 1 / (P - 2) sum_p |Y_p / X - H[.., 0, :] - (-1)^p H[.., 1, :]|^2
  weights(vars, p)                       -> w [B, F, C] through diversity_ref.noise_weights
  detect_mimo / detect_stbc(.., w, p)    -> the unweighted restatements on Y_b sqrt(w_b), H_b sqrt(w_b)
  branch_snr_db, mimo_snr_db, stbc_snr_db -> what the receive calls publish
  receive_mimo / receive_stbc(recordings, p, advance) -> the whole chains, weighted and unweighted
  coloured(recordings, tx2, snr_db, p)   -> the scenario's noise: 6 x in amplitude in one band per microphone

The weighted metric sum_b w_b |y_b - h_b0 x0 - h_b1 x1|^2 is the unweighted one on y_b sqrt(w_b) and h_bt sqrt(w_b); the
oracle's channel model interpolates the magnitudes of the start and end estimates linearly and leaves their phases alone,
so scaling both estimates by sqrt(w_b) scales every channel entry by it."""
import numpy as np

from tests import diversity_ref as DR
from tests import mimo_ref as MR
from tests import stbc_ref as SR


# ---- the estimate --------------------------------------------------------------------------------------------------------
def pilot_terms(x, starts, H, p):
    """-> (q [F, 2, P, K] = Y_p / X of both pilot blocks, e [F, 2, P, K] = q - H0 - (-1)^p H1, status [F]); NaN rows and
    status 1 for a packet whose body leaves [0, len(x)) at either end (mimo_ref.pilots' rule)."""
    if p.P < 4 or p.P % 2:
        raise ValueError(f"the noise is measured on the pilot symbols the two covers leave over: an even P >= 4, not {p.P}")
    x = np.asarray(x, dtype=np.float64)
    H = np.asarray(H, dtype=complex)
    F = len(starts)
    q = np.full((F, 2, p.P, p.K), complex(np.nan, np.nan))
    status = np.zeros(F, dtype=np.int32)
    kn = p.known_symbols()
    car = np.arange(1, p.K + 1)
    L = p.M * p.S
    for f, s in enumerate(np.asarray(starts, dtype=np.int64)):
        if s < 0 or s + L > len(x):
            status[f] = 1
            continue
        X = np.fft.fft(x[s: s + L].reshape(p.M, p.S)[:, p.CP:])
        q[f, 0], q[f, 1] = X[:p.P, car] / kn, X[p.P + p.D:, car] / kn
    sign = MR.cover(p.P)[1][None, None, :, None]
    with np.errstate(invalid="ignore"):
        e = q - H[:, :, 0][:, :, None, :] - sign * H[:, :, 1][:, :, None, :]
    return q, e, status


def pilot_noise(x, starts, H, p):
    """-> (v float64 [F, 2, K], status int32 [F]), p ascending in the sum"""
    _, e, status = pilot_terms(x, starts, H, p)
    v = np.zeros(e.shape[:2] + e.shape[3:])
    for i in range(p.P):
        v = v + (e[:, :, i].real ** 2 + e[:, :, i].imag ** 2)
    return v / (p.P - 2), status


# ---- the rule ------------------------------------------------------------------------------------------------------------
def carrier_vars(vars_, p):
    """B arrays [F, 2, K] -> [B, F, C]: the mean of the two sides at every data carrier's bin"""
    col = p.data_carriers - 1
    return np.stack([0.5 * (np.asarray(v)[:, 0, col] + np.asarray(v)[:, 1, col]) for v in vars_])


def weights(vars_, p):
    return DR.noise_weights(carrier_vars(vars_, p))


# ---- the detectors -------------------------------------------------------------------------------------------------------
def scaled(Ys, Hs, w, p):
    """Y_b sqrt(w_b) on the data carriers' bins and H_b sqrt(w_b) on their columns; a weight that is not finite counts as 0"""
    col = p.data_carriers - 1
    Yw, Hw = [], []
    for Y, H, wb in zip(Ys, Hs, np.asarray(w, dtype=np.float64)):
        r = np.sqrt(np.where(np.isfinite(wb) & (wb > 0), wb, 0.0))             # [F, C]
        F = r.shape[0]
        Y = np.array(Y, dtype=complex).reshape(F, p.D, p.N // 2 + 1)
        H = np.array(H, dtype=complex)
        Y[:, :, p.data_carriers] = np.where(r[:, None, :] == 0, 0.0, Y[:, :, p.data_carriers] * r[:, None, :])
        H[:, :, :, col] = np.where(r[:, None, None, :] == 0, 0.0, H[:, :, :, col] * r[:, None, None, :])
        Yw.append(Y.reshape(F * p.D, -1))
        Hw.append(H)
    return Yw, Hw


def detect_mimo(Ys, Hs, slopes, w, p):
    return MR.detect(*scaled(Ys, Hs, w, p), slopes, p)


def detect_stbc(Ys, Hs, slope, w, p):
    return SR.detect(*scaled(Ys, Hs, w, p), slope, p)


# ---- what the receive calls publish --------------------------------------------------------------------------------------
def start_estimates(Hs, p):
    """[B, F, 2 speakers, C]: the start-block estimates on the data carriers"""
    return np.stack([np.asarray(H)[:, 0] for H in Hs])[..., p.data_carriers - 1]


def branch_snr_db(Hs, vars_, p):
    es = np.mean(np.abs(p.const_points) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(es * np.abs(start_estimates(Hs, p)) ** 2 / DR.floored_all(carrier_vars(vars_, p))[:, :, None, :])


def mimo_snr_db(Hs, w, p):
    """[F, 2, C]: the zero-forcing SNR of either stream from the weighted sums"""
    es, h = np.mean(np.abs(p.const_points) ** 2), start_estimates(Hs, p)
    g = [(w * np.abs(h[:, :, t]) ** 2).sum(axis=0) for t in range(2)]
    g01 = np.abs((w * np.conj(h[:, :, 0]) * h[:, :, 1]).sum(axis=0)) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(es * np.stack([g[0] - g01 / g[1], g[1] - g01 / g[0]], axis=1))


def stbc_snr_db(Hs, w, p):
    es, h = np.mean(np.abs(p.const_points) ** 2), start_estimates(Hs, p)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(es * (w * (np.abs(h) ** 2).sum(axis=2)).sum(axis=0))


# ---- the whole chains ------------------------------------------------------------------------------------------------------
def _weighted(o, recordings, p, advance):
    vars_ = []
    for r, st in zip(recordings, o["starts"]):
        v, status = pilot_noise(r, st - advance, o["H"][len(vars_)], p)
        assert not status.any()
        vars_.append(v)
    return vars_, weights(vars_, p)


def receive_mimo(recordings, p, advance=48):
    """mimo_ref.receive_mimo (the unweighted chain: "llr", "bits") and on its sync, estimates and spectra the weighted one:
    "vars", "w", "llr_w", "bits_w", "snr_db", "branch_snr_db"."""
    o = MR.receive_mimo(recordings, p, advance)
    vars_, w = _weighted(o, recordings, p, advance)
    llr, _ = detect_mimo(o["Y"], o["H"], o["slopes"], w, p)
    o.update(vars=vars_, w=w, llr_w=llr.reshape(-1), bits_w=(llr.reshape(-1) < 0).astype(np.int64),
             snr_db=mimo_snr_db(o["H"], w, p), branch_snr_db=branch_snr_db(o["H"], vars_, p))
    return o


def receive_stbc(recordings, p, advance=48):
    """stbc_ref.receive_stbc and the weighted chain on its sync, estimates, slope and spectra; keys as receive_mimo's."""
    o = SR.receive_stbc(recordings, p, advance)
    vars_, w = _weighted(o, recordings, p, advance)
    llr, _ = detect_stbc(o["Y"], o["H"], o["slope"], w, p)
    o.update(vars=vars_, w=w, llr_w=llr.reshape(-1), bits_w=(llr.reshape(-1) < 0).astype(np.int64),
             snr_db=stbc_snr_db(o["H"], w, p), branch_snr_db=branch_snr_db(o["H"], vars_, p))
    return o


# ---- the scenario's noise ------------------------------------------------------------------------------------------------
BANDS = ((0, 150), (250, 512))      # microphone b's noisy band [lo, hi), in carrier bins of the parameters' transform
BOOST = 6.0


def coloured(recordings, tx2, snr_db, p, boost=BOOST, mics=None):
    """Gaussian noise snr_db below stbc_ref.body_rms(tx2), seed 20 + b at microphone b, `boost` x in amplitude where the
    frequency i / (len - 1) * (N / 2) of rfft bin i lies in BANDS[b] (boost = 1: white)."""
    sigma = SR.body_rms(tx2) * 10.0 ** (-snr_db / 20.0)
    out = []
    for r, b in zip(recordings, range(len(recordings)) if mics is None else mics):
        n = len(r)
        spec = np.fft.rfft(np.random.default_rng(20 + b).normal(size=n))
        at = np.arange(len(spec)) / (len(spec) - 1) * (p.N / 2)
        g = np.where((at >= BANDS[b][0]) & (at < BANDS[b][1]), boost, 1.0) if b < len(BANDS) else np.ones(len(spec))
        out.append(r + sigma * np.fft.irfft(spec * g, n))
    return out
