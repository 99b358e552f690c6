"""NumPy restatement of the impulse blanking ahead of the demodulator (gf3_blank_impulses), written from its definition.

The body of packet f is its M symbols of S samples, [s_f, s_f + M S).  Per symbol, over the finite samples: mean and
energy = max(sum v^2 / n - mean^2, 0) in fp64 (no finite sample: +Inf and 0).  The symbol of rank (M - 1) // 4 among the
energies (ascending, ties to the lower index) gives the packet's baseline mu and sigma = sqrt(energy); T = kappa sigma.  A
sample is flagged if it is not finite or |v - mu| > T (strict), blanked if a flagged sample of the same body lies within
`guard` samples, and a blanked sample becomes mu in the storage type.  A packet whose body is not inside the stream writes
nothing and reports counts -1, energy 0, level (0, 0)."""
import numpy as np


def rank_of(M):
    return (M - 1) // 4


def pick(energy):
    """Index of the symbol at rank (M - 1) // 4 in ascending order of energy, ties to the lower index."""
    order = np.argsort(np.asarray(energy, dtype=np.float64), kind="stable")
    return int(order[rank_of(len(order))])


def symbol_stats(v):
    """(mean, energy, sum v^2 / n) of one symbol's samples (already widened to fp64)."""
    fin = v[np.isfinite(v)]
    if fin.size == 0:
        return 0.0, np.inf, 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        mean = fin.sum() / fin.size
        ms = (fin * fin).sum() / fin.size
        e = ms - mean * mean
    return float(mean), float(e) if e > 0 else 0.0, float(ms)


def to_storage(mu, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return dtype.type(min(max(np.rint(mu), info.min), info.max))
    return dtype.type(mu)


def blank(x, starts, M, S, kappa=4.5, guard=8, out=None, details=False):
    """-> (out, counts [F, M] int32, level [F, 2] float64, energy [F, M] float64); with details a dict more: "flags" and
    "blanked" (one boolean array of M S per packet, None for a ragged one), "margin" (the smallest | |v - mu| - T | / T over
    the finite samples of the packets with finite T > 0), "half" (the smallest distance of a mu from a half-integer) and
    "meansq" [F, M] (sum v^2 / n per symbol, the scale of the tolerance on energy).
    out: what the caller filled the second buffer with (a copy of x when absent); it is copied, not written."""
    x = np.asarray(x)
    out = x.copy() if out is None else np.array(out, dtype=x.dtype)
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    F, n, L = len(starts), len(x), M * S
    counts = np.zeros((F, M), dtype=np.int32)
    level = np.zeros((F, 2))
    energy = np.zeros((F, M))
    det = {"flags": [], "blanked": [], "margin": np.inf, "half": np.inf, "meansq": np.zeros((F, M))}
    for f, s in enumerate(starts):
        if s < 0 or s + L > n:
            counts[f] = -1
            det["flags"].append(None)
            det["blanked"].append(None)
            continue
        v = x[s: s + L].astype(np.float64)
        means = np.zeros(M)
        for m in range(M):
            means[m], energy[f, m], det["meansq"][f, m] = symbol_stats(v[m * S: (m + 1) * S])
        m0 = pick(energy[f])
        mu = means[m0] if np.isfinite(means[m0]) else 0.0
        sigma = np.sqrt(energy[f, m0])
        level[f] = mu, sigma
        T = kappa * sigma
        fin = np.isfinite(v)
        with np.errstate(invalid="ignore"):
            dev = np.abs(v - mu)
            flags = ~fin | (dev > T)
        idx = np.flatnonzero(flags)
        blanked = np.zeros(L, dtype=bool)
        for j in idx:                                    # the guard stays inside the body
            blanked[max(j - guard, 0): min(j + guard, L - 1) + 1] = True
        out[s: s + L][blanked] = to_storage(mu, x.dtype)
        counts[f] = blanked.reshape(M, S).sum(axis=1)
        det["flags"].append(flags)
        det["blanked"].append(blanked)
        if np.isfinite(T) and T > 0 and fin.any():
            det["margin"] = min(det["margin"], float(np.abs(dev[fin] - T).min() / T))
        det["half"] = min(det["half"], float(abs(abs(mu - np.floor(mu)) - 0.5)))
    res = (out, counts, level, energy)
    return res + (det,) if details else res


def click_scenario(sig, body_start, p_M, S, P, D, share, amplitude, rng, length=200, pilots=(3, 11)):
    """The issue's click scenario on a clean stream: a burst of `length` samples of white noise at `amplitude` x the body's
    rms at a random place inside `share` of the data symbols and inside the start pilots `pilots`.
    -> (the clicks to add, the body-symbol numbers that were hit, sorted)"""
    body = sig[body_start: body_start + p_M * S]
    rms = float(np.sqrt(np.mean(body ** 2)))
    hit = sorted(list(pilots) + [P + int(i) for i in rng.choice(D, size=int(round(share * D)), replace=False)])
    clicks = np.zeros_like(sig, dtype=np.float64)
    for m in hit:
        at = body_start + m * S + int(rng.integers(0, S - length))
        clicks[at: at + length] = rng.normal(0.0, amplitude * rms, length)
    return clicks, hit
