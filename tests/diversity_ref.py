"""NumPy restatement of receive diversity ("Receive diversity"), written from the definition, not from the
kernel.  B branches hold the equalised symbols of B recordings of one transmission, eq_b [F*D, C]:

  1. weights, csi:    w_b[f,l,c] = (|Hs_b| + (|He_b| - |Hs_b|) (l + P/2) / (D + P))^2 at the carrier's bin (Hs, He [F, K])
     weights, noise:  vbar[f] = mean over b and c of var_b[f,c];  w_b[f,c] = 1 / max(var_b, 1e-6 vbar); 1 for the whole
                      packet where vbar is 0 or not finite (var_b [F, C] from noise_ref.noise_estimate on branch b)
     either:          w_b = 0 where its input or the weight is not finite, or where eq_b is not finite in either part
  2. W = sum_b w_b;  z = (sum_b w_b eq_b) / W, summed for b ascending;  z = 0 where W = 0
  3. LLR = maxlog(z; sigma^2 = 1) W, float32; +0 where W = 0
  4. branch SNR [B, F, C] = 10 log10(Es / max(var_b, 1e-6 vbar)), combined SNR [F, C] = 10 log10(Es sum_b w_b) with the
     weights of step 1 before the per-symbol zeroing (noise weights only)

and the two-microphone scenario the tests share (`two_paths`, `add_noise`, `single_llrs`, `failed`)."""
import numpy as np

from tests import noise_ref as NR


def csi_weights(Hs, He, bins, P, D):
    """Hs, He [F, K], bins: 1-based FFT bins of the data carriers -> [F, D, C]; 0 where |Hs| or |He| is not finite"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.abs(np.asarray(Hs))[:, None, np.asarray(bins) - 1]
        e = np.abs(np.asarray(He))[:, None, np.asarray(bins) - 1]
        frac = ((np.arange(D) + P / 2.0) / (D + P))[None, :, None]
        w = (s + (e - s) * frac) ** 2
    return np.where(np.isfinite(s) & np.isfinite(e) & np.isfinite(w), w, 0.0)


def floored_all(vars_):
    """[B, F, C] -> max(var_b, 1e-6 vbar), vbar the mean over all branches and carriers of the packet"""
    v = np.asarray(vars_, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.maximum(v, 1e-6 * v.mean(axis=(0, 2))[None, :, None])


def noise_weights(vars_):
    """B arrays [F, C] -> [B, F, C]"""
    v = np.asarray(vars_, dtype=np.float64)
    vbar = v.mean(axis=(0, 2))[None, :, None]
    flat = ~(np.isfinite(vbar) & (vbar > 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(flat, 1.0, 1.0 / floored_all(v))
    return np.where(np.isfinite(v) & np.isfinite(w), w, 0.0)


def per_symbol(w, D):
    """noise weights [B, F, C] -> [B, F*D, C]; csi weights [B, F, D, C] -> the same shape"""
    w = np.asarray(w)
    if w.ndim == 3:
        w = np.repeat(w[:, :, None, :], D, axis=2)
    return w.reshape(w.shape[0], -1, w.shape[-1])


def combine(eqs, w):
    """eqs [B, F*D, C], w [B, F*D, C] -> (z [F*D, C], W [F*D, C])"""
    eqs = np.asarray(eqs, dtype=np.complex128)
    w = np.where(np.isfinite(eqs.real) & np.isfinite(eqs.imag), w, 0.0)
    acc = np.zeros(eqs.shape[1:], dtype=np.complex128)
    W = np.zeros(eqs.shape[1:])
    for b in range(eqs.shape[0]):
        acc = acc + np.where(w[b] == 0, 0.0, w[b] * np.where(w[b] == 0, 0.0, eqs[b]))
        W = W + w[b]
    with np.errstate(divide="ignore", invalid="ignore"):
        Wd = np.where(W == 0, 1.0, W)
        z = np.where(W == 0, 0.0, acc.real / Wd + 1j * (acc.imag / Wd))
    return z, W


def llrs(z, W, points, bits):
    """-> float32 [F*D*C*mu]"""
    with np.errstate(invalid="ignore", over="ignore"):
        out = NR.maxlog(z, points, bits) * W[..., None]
    return np.where(W[..., None] == 0, 0.0, out).astype(np.float32).reshape(-1)


def combine_csi(eqs, Hs, He, bins, P, D, points, bits):
    w = per_symbol([csi_weights(h, g, bins, P, D) for h, g in zip(Hs, He)], D)
    z, W = combine(eqs, w)
    return z, W, llrs(z, W, points, bits)


def combine_noise(eqs, vars_, D, points, bits):
    z, W = combine(eqs, per_symbol(noise_weights(vars_), D))
    return z, W, llrs(z, W, points, bits)


def branch_snr_db(vars_, points):
    es = np.mean(np.abs(points) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(es / floored_all(vars_))


def combined_snr_db(vars_, points):
    es = np.mean(np.abs(points) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(es * noise_weights(vars_).sum(axis=0))


# ---- the two-microphone scenario -------------------------------------------------------------------------------------
H0 = (12, 0.9)          # branch 0: h = delta[n] + 0.9 delta[n - 12]
H1 = (17, -0.9)         # branch 1: h = delta[n] - 0.9 delta[n - 17], and the recording starts DELAY samples later
DELAY = 5
SEEDS = (10, 11)


def two_paths(tx):
    """The clean transmitted stream through the two rooms -> [branch 0, branch 1] (noiseless)."""
    out = []
    for (lag, g), delay in ((H0, 0), (H1, DELAY)):
        h = np.zeros(lag + 1)
        h[0], h[lag] = 1.0, g
        out.append(np.concatenate([np.zeros(delay), np.convolve(tx, h)]))
    return out


def add_noise(branches, tx, snr_db, scale=1.0):
    """White Gaussian noise, seeds 10 and 11, of amplitude `scale` x (snr_db below the RMS of the transmitted stream)."""
    sigma = scale * np.sqrt(np.mean(np.asarray(tx) ** 2)) * 10.0 ** (-snr_db / 20.0)
    return [b + sigma * np.random.default_rng(s).normal(size=len(b)) for b, s in zip(branches, SEEDS)]


def single_llrs(o, weighting, p):
    """One branch alone: the oracle's demodulator outputs -> the LLRs receive() would form under `weighting`"""
    if weighting == "csi":
        w = csi_weights(o["Hs"], o["He"], p.data_carriers, p.P, p.D).reshape(-1, p.C)
        return (NR.maxlog(o["eq"], p.const_points, p.const_bits) * w[..., None]).astype(np.float32).reshape(-1)
    return NR.soft_demap_nw(o["eq"], NR.noise_estimate(o["eq"], p.const_points, p.D), p.const_points, p.const_bits, p.D)


def failed(sh, llr, msg, max_iter=50):
    """Codewords of msg [n_cw, k] the restated decoder does not return from `llr` (given up or wrong)"""
    from tests import ldpc_ref as R
    n_cw, n = msg.shape[0], sh.shape[1] * 64
    bits, _, it = R.decode(sh, np.asarray(llr[: n_cw * n], dtype=np.float32).reshape(n_cw, n), max_iter)
    return int(np.sum((bits != msg).any(axis=1) | (it < 0)))
