"""NumPy restatement of the decision-directed noise estimate and the noise-weighted soft demapper,
written from the definition, not from the kernels:

  1. e[f,l,c] = eq - s, s the constellation point `demap` picks: argmin of abs(eq - table), first minimum (in-order scan,
     strict <; NaN / Inf decide point 0)
  2. v[f,c]   = (1/D) sum_l |e|^2                                  (fp64)
  3. vbar[f]  = mean_c v[f,c];  v'[f,c] = max(v[f,c], 1e-6 vbar[f])
     w[f,c]   = 0 where v[f,c] is not finite, else 1 for the whole packet where vbar[f] is 0 or not finite, else 1 / v'
  4. LLR      = maxlog(eq; sigma^2 = 1) * w, float32; +0 where w = 0 (an erasure, whatever the symbol held)
  5. snr_db   = 10 log10(Es / v'), Es the mean energy of the table (plain IEEE: +inf on a noiseless carrier)

eq is [F*D, C] as demod_frames returns it (packet -> symbol -> carrier)."""
import numpy as np


def decide(eq, points):
    """Index of the point the reference's demap picks."""
    with np.errstate(invalid="ignore"):
        return np.abs(eq[..., None] - points).argmin(axis=-1)


def noise_estimate(eq, points, D):
    eq = np.asarray(eq, dtype=np.complex128)
    C = eq.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        e = eq - points[decide(eq, points)]
        p = (e.real ** 2 + e.imag ** 2).reshape(-1, D, C)
        return p.sum(axis=1) / D


def floored(var):
    with np.errstate(invalid="ignore"):
        return np.maximum(var, 1e-6 * var.mean(axis=1, keepdims=True))


def weights(var):
    var = np.asarray(var, dtype=np.float64)
    vbar = var.mean(axis=1, keepdims=True)
    flat = ~(np.isfinite(vbar) & (vbar > 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(flat, 1.0, 1.0 / floored(var))
    return np.where(np.isfinite(var), w, 0.0)


def maxlog(eq, points, bits):
    """max-log LLR at sigma^2 = 1 per bit, [..., mu]; LLR > 0 <=> bit 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = np.abs(eq[..., None] - points) ** 2
        out = np.empty(eq.shape + (bits.shape[1],))
        for b in range(bits.shape[1]):
            out[..., b] = d2[..., bits[:, b] == 1].min(axis=-1) - d2[..., bits[:, b] == 0].min(axis=-1)
    return out


def soft_demap_nw(eq, var, points, bits, D):
    """-> float32 [F*D*C*mu]"""
    eq = np.asarray(eq, dtype=np.complex128)
    C = eq.shape[-1]
    w = np.repeat(weights(var), D, axis=0).reshape(eq.shape)           # [F*D, C]
    with np.errstate(invalid="ignore", over="ignore"):
        llr = maxlog(eq, points, bits) * w[..., None]
    return np.where(w[..., None] == 0, 0.0, llr).astype(np.float32).reshape(-1)


def snr_db(var, points):
    es = np.mean(np.abs(points) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(es / floored(np.asarray(var, dtype=np.float64)))
