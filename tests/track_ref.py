"""NumPy restatement of the per-symbol phase and timing tracker, written from the
definition, not from the kernel.

eq is [F*D, C] as demod_frames returns it (packet -> symbol -> carrier); `bins` are the context's data bins k_c (1-based,
any order), kappa_c = k_c - mean(k).  Every packet starts at a = b = va = vb = 0; per symbol l

  1. pa = a + va, pb = b + vb
  2. z_c = eq[l, c] exp(-i (pa + pb kappa_c))
  3. a carrier whose z_c is not finite in both parts is left out of every sum; else s_c = the point `demap` picks for z_c
     (noise_ref.decide: in-order scan, strict <) and r_c = z_c conj(s_c)
  4. S0 = sum r, S1 = sum kappa r, S2 = sum kappa^2 r, E = sum |z - s|^2, P = sum |s|^2          (fp64)
  5. da = atan2(Im S0, Re S0) (0 for S0 = 0), u = exp(-i da), den = Re(u S2);
     measured <=> every sum finite, den > 0 and E <= P:  na = pa + da, nb = pb + Im(u S1) / den;  else na = pa, nb = pb
  6. va = na - a, vb = nb - b, a = na, b = nb
  7. out[l, c] = eq[l, c] exp(-i (a + b kappa_c)),  phase[f, l] = (a, b),  measured[f, l] = 0 / 1
"""
import numpy as np

from tests.noise_ref import decide


def kappa(bins):
    k = np.asarray(bins, dtype=np.float64)
    return k - k.mean()


def track(eq, points, bins, D, velocity=True, details=False):
    """-> (out [F*D, C] complex128, phase [F, D, 2] float64, measured [F, D] uint8[, details]).
    velocity=False drops step 1's prediction (pa = a, pb = b): what the loop would be without its velocity term.
    details: dict of per-symbol [F, D] arrays -- `margin`: the smallest (second-nearest - nearest) distance over the
    carriers that entered the sums (inf when none did), `E`, `P`, `den`, `k2r` = sum kappa^2 |r|, `finite`."""
    eq = np.asarray(eq, dtype=np.complex128)
    points = np.asarray(points, dtype=np.complex128)
    C = eq.shape[-1]
    F = eq.shape[0] // D
    kap = kappa(bins)
    assert kap.shape == (C,) and eq.shape == (F * D, C)
    out = np.empty_like(eq)
    phase = np.zeros((F, D, 2))
    measured = np.zeros((F, D), dtype=np.uint8)
    det = {k: np.zeros((F, D)) for k in ("margin", "E", "P", "den", "k2r")}
    det["finite"] = np.zeros((F, D), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for f in range(F):
            a = b = va = vb = 0.0
            for l in range(D):
                row = eq[f * D + l]
                pa, pb = (a + va, b + vb) if velocity else (a, b)
                z = row * np.exp(-1j * (pa + pb * kap))
                ok = np.isfinite(z.real) & np.isfinite(z.imag)
                zk, kk = z[ok], kap[ok]
                s = points[decide(zk, points)]
                r = zk * np.conj(s)
                S0, S1, S2 = r.sum(), (kk * r).sum(), (kk * kk * r).sum()
                d = zk - s
                E = (d.real ** 2 + d.imag ** 2).sum()
                P = (s.real ** 2 + s.imag ** 2).sum()
                da = 0.0 if S0 == 0 else float(np.arctan2(S0.imag, S0.real))
                u = np.exp(-1j * da)
                den = (u * S2).real
                fin = bool(np.isfinite([S0.real, S0.imag, S1.real, S1.imag, S2.real, S2.imag, E, P]).all())
                m = fin and den > 0 and E <= P
                na, nb = (pa + da, pb + (u * S1).imag / den) if m else (pa, pb)
                va, vb, a, b = na - a, nb - b, na, nb
                out[f * D + l] = row * np.exp(-1j * (a + b * kap))
                phase[f, l] = a, b
                measured[f, l] = m
                if details:
                    dist = np.sort(np.abs(zk[:, None] - points), axis=1)
                    det["margin"][f, l] = (dist[:, 1] - dist[:, 0]).min() if len(zk) and len(points) > 1 else np.inf
                    det["E"][f, l], det["P"][f, l], det["den"][f, l] = E, P, den
                    det["k2r"][f, l] = (kk * kk * np.abs(r)).sum()
                    det["finite"][f, l] = fin
    return (out, phase, measured, det) if details else (out, phase, measured)


def robust(det, tol=1e-6):
    """Which symbols' gates are decided by a margin (the GPU test's precondition) -> (measured, coasting) boolean [F, D]:
    measured: sums finite, den > tol k2r and E < P (1 - tol);  coasting: a sum is not finite, or E > P (1 + tol), or
    k2r = 0 exactly (nothing entered the sums, every symbol zero, or kappa = 0: den = 0 on any summation order)."""
    fin = det["finite"]
    with np.errstate(invalid="ignore"):
        meas = fin & (det["den"] > tol * det["k2r"]) & (det["k2r"] > 0) & (det["E"] < det["P"] * (1 - tol))
        coast = ~fin | (det["E"] > det["P"] * (1 + tol)) | (det["k2r"] == 0)
    return meas, coast


# ---- test inputs ---------------------------------------------------------------------------------------------------
def swing(D, peak):
    """peak sin^2(pi (l + 1/2) / D): zero at both ends of the packet, where the pilots sit."""
    return peak * np.sin(np.pi * (np.arange(D) + 0.5) / D) ** 2


def delay_wander(sig, first, S, D, tau0):
    """The stream with every data symbol's block of S samples (prefix included; symbol l starts at first + l S) delayed
    circularly, through its S-point real FFT, by tau_l = tau0 sin^2(pi (l + 1/2) / D) samples."""
    out = np.array(sig, dtype=np.float64)
    k = np.arange(S // 2 + 1)
    for l, tau in enumerate(swing(D, tau0)):
        blk = out[first + l * S: first + (l + 1) * S]
        blk[:] = np.fft.irfft(np.fft.rfft(blk) * np.exp(-2j * np.pi * k * tau / S), S)
    return out
