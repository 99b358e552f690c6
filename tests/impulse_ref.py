"""NumPy restatement of the impulse-noise pair: carrier x symbol noise weights and the packet interleaver,
written from the definition, not from the kernels:

  1. e[f,l,c]  = eq - s, s chosen as noise_ref.decide does
  2. v_c[f,c]  = (1/D) sum_l |e|^2   (noise_ref.noise_estimate);   v_s[f,l] = (1/C) sum_c |e|^2   (fp64)
  3. vbar[f]   = mean_c v_c[f,c];  w[f,l,c] = 1 / max(v_c v_s / vbar, 1e-6 vbar);
     w = 0 where v_c[f,c] or v_s[f,l] is not finite, otherwise 1 for the whole packet where vbar is 0 or not finite
  4. LLR       = maxlog(eq; sigma^2 = 1) * w, float32; +0 where w = 0
  5. snr_db_s  = 10 log10(Es / max(v_s, 1e-6 vbar))
  6. interleaver on a packet's nbp = D C mu coded bits: coded bit i is transmitted at pi(i) = (i s) mod nbp, s the smallest
     integer >= C mu + 1 with gcd(s, nbp) = 1

eq is [F*D, C] as demod_frames returns it (packet -> symbol -> carrier)."""
from math import gcd

import numpy as np

from tests import noise_ref as NR


def noise_estimate2(eq, points, D):
    """-> (v_c [F, C], v_s [F, D])"""
    eq = np.asarray(eq, dtype=np.complex128)
    C = eq.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        e = eq - points[NR.decide(eq, points)]
        p = (e.real ** 2 + e.imag ** 2).reshape(-1, D, C)
        return p.sum(axis=1) / D, p.sum(axis=2) / C


def weights2(var_c, var_s):
    """-> w [F, D, C]"""
    var_c = np.asarray(var_c, dtype=np.float64)
    var_s = np.asarray(var_s, dtype=np.float64)
    vbar = var_c.mean(axis=1)[:, None, None]
    flat = ~(np.isfinite(vbar) & (vbar > 0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x = var_c[:, None, :] * var_s[:, :, None] / vbar
        w = np.where(flat, 1.0, 1.0 / np.maximum(x, 1e-6 * vbar))
    return np.where(np.isfinite(var_c)[:, None, :] & np.isfinite(var_s)[:, :, None], w, 0.0)


def soft_demap_nw2(eq, var_c, var_s, points, bits):
    """-> float32 [F*D*C*mu], transmitted order"""
    eq = np.asarray(eq, dtype=np.complex128)
    w = weights2(var_c, var_s).reshape(eq.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        llr = NR.maxlog(eq, points, bits) * w[..., None]
    return np.where(w[..., None] == 0, 0.0, llr).astype(np.float32).reshape(-1)


def symbol_snr_db(var_c, var_s, points):
    es = np.mean(np.abs(points) ** 2)
    var_c = np.asarray(var_c, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(es / np.maximum(np.asarray(var_s, dtype=np.float64), 1e-6 * var_c.mean(axis=1, keepdims=True)))


def stride(B, nbp):
    s = B + 1
    while gcd(s, nbp) != 1:
        s += 1
    return s


def perm(D, C, mu):
    """pi as an index array: coded bit i travels at position perm[i]  (Python integers: i s needs more than 32 bits)"""
    nbp = D * C * mu
    s = stride(C * mu, nbp)
    return np.array([(i * s) % nbp for i in range(nbp)], dtype=np.int64)


def interleave(x, D, C, mu):
    """[..., nbp] coded order -> transmitted order"""
    x = np.asarray(x)
    out = np.empty_like(x)
    out[..., perm(D, C, mu)] = x
    return out


def deinterleave(x, D, C, mu):
    """[..., nbp] transmitted order -> coded order"""
    return np.asarray(x)[..., perm(D, C, mu)]
