"""NumPy restatement of the delay-domain pilot denoiser (gf3_denoise_pilots, include/gf3rx.h) -- TEST
INFRASTRUCTURE.  It is the reference the kernel is held to, and the rule itself:

per packet and per side, tau = threshold, x_p[n] the N samples after the prefix of pilot symbol p = 0 .. P-1,
    S[n] = sum_p x_p[n]                                    (added in order of p, from 0.0: the two-phase form's pilot sum)
    v    = sum_n sum_p (x_p[n] - S[n]/P)^2 / ((P-1) N)
    H_k  = rfft(S)_k / (P kn_k), k = 1 .. K;  H_0 = H_{N/2} = 0;  h = irfft(H)
    s2   = 2 v / (N P) sum_k 1/|kn_k|^2
    keep tap n iff h[n]^2 > tau s2;  kept, post (largest kept n < N/2, else -1), pre (largest N - n over kept n >= N/2, else 0)
    pass-through (row unchanged, applied = 0): v not finite, ragged packet (zero row; v = 0, kept = 0, post = -1, pre = 0),
    kept > N/4
    else S' = irfft(X'), X'_k = rfft(h keep)_k P kn_k (k = 1 .. K), X'_0, X'_{N/2} as in rfft(S); applied = 1
report = (v, kept, post, pre, applied)."""
import numpy as np

REPORT = ("v", "kept", "post", "pre", "applied")


def pilot_sum(xp):
    """[P, N] pilot symbols -> their sum, added in order of p from 0.0 (pilot_sum_kernel's order)."""
    s = np.zeros(xp.shape[1])
    for p in range(xp.shape[0]):
        s = s + xp[p]
    return s


def taps(S, P, kn):
    """h = irfft(rfft(S) / (P kn)) with bins 0 and N/2 zero, and the spectrum X = rfft(S)."""
    N = len(S)
    X = np.fft.rfft(S)
    H = np.zeros(N // 2 + 1, dtype=complex)
    H[1:N // 2] = X[1:N // 2] / (P * kn)
    return np.fft.irfft(H, N), X


def tap_variance(v, N, P, kn):
    return 2.0 * v / (N * P) * np.sum(1.0 / np.abs(kn) ** 2)


def denoise_row(xp, kn, tau=9.0, max_kept=None):
    """One (packet, side): xp [P, N] float64 pilot symbols without their prefixes, kn [K] known symbols.
    -> (S' [N], report [5], margin): margin = min_n |h[n]^2 / (tau s2) - 1| (inf where no threshold was formed): how far the
    nearest tap is from the keep decision.  max_kept: the pass-through bound on `kept`, N/4 unless a test forces another."""
    xp = np.asarray(xp, dtype=np.float64)
    P, N = xp.shape
    assert P >= 2
    max_kept = N // 4 if max_kept is None else max_kept
    S = pilot_sum(xp)
    with np.errstate(invalid="ignore", over="ignore"):
        d = xp - S / P
        v = np.sum(d * d) / ((P - 1) * N)
    if not np.isfinite(v):
        return S, np.array([v, 0.0, -1.0, 0.0, 0.0]), np.inf
    h, X = taps(S, P, kn)
    thr = tau * tap_variance(v, N, P, kn)
    keep = h * h > thr
    margin = np.min(np.abs(h * h / thr - 1.0)) if thr > 0 else np.inf
    idx = np.flatnonzero(keep)
    kept = len(idx)
    lo, hi = idx[idx < N // 2], idx[idx >= N // 2]
    post = int(lo.max()) if len(lo) else -1
    pre = int((N - hi).max()) if len(hi) else 0
    if kept > max_kept:
        return S, np.array([v, kept, post, pre, 0.0]), margin
    H2 = np.fft.rfft(h * keep)
    X2 = X.copy()
    X2[1:N // 2] = H2[1:N // 2] * (P * kn)
    return np.fft.irfft(X2, N), np.array([v, kept, post, pre, 1.0]), margin


def denoise_frames(x, offsets, N, CP, P, D, kn, tau=9.0):
    """The stage on a stream: x samples (any storage type), offsets [F] of each packet's first pilot prefix.
    -> (psum' [F, 2, N], report [F, 2, 5], psum [F, 2, N] plain pilot sums, margin: the smallest over all rows)."""
    x = np.asarray(x)
    S_ = N + CP
    F = len(offsets)
    out, plain, rep = np.zeros((F, 2, N)), np.zeros((F, 2, N)), np.zeros((F, 2, 5))
    margin = np.inf
    for f, off in enumerate(offsets):
        if off < 0 or off + (2 * P + D) * S_ > len(x):
            rep[f, :] = (0.0, 0.0, -1.0, 0.0, 0.0)
            continue
        for side in range(2):
            base = off + (side * (P + D)) * S_
            xp = np.stack([x[base + p * S_ + CP: base + (p + 1) * S_] for p in range(P)]).astype(np.float64)
            plain[f, side] = pilot_sum(xp)
            out[f, side], rep[f, side], m = denoise_row(xp, kn, tau)
            margin = min(margin, m)
    return out, rep, plain, margin


def sparse_channel(rng, ntaps, decay):
    """Gaussian taps of amplitude exp(-n / decay), made DC- and Nyquist-free (h[n] - h[n-2]), unit energy."""
    g = rng.standard_normal(ntaps) * np.exp(-np.arange(ntaps) / decay)
    h = np.zeros(ntaps + 2)
    h[:ntaps] += g
    h[2:] -= g
    return h / np.sqrt(np.sum(h * h))


# ---- inputs shared by tests/test_denoise_cpu.py and tests/test_denoise_gpu.py ---------------------------------------
def small_params(known_bits):
    """The small geometry of the end-to-end tests: N = 1024, CP = 64, P = 2, D = 12, carriers 20 .. 399, fit over [100, 300)."""
    from oracle import gf3_oracle as orc
    pts, bits = orc.qpsk_table()
    return orc.RxParams(N=1024, CP=64, P=2, D=12, lo=20, hi=400, fit_lo=100, fit_hi=300, const_points=pts, const_bits=bits,
                        known_bits=np.asarray(known_bits, dtype=np.uint8))


def noisy_stream(p, seed, ntaps=24, decay=5.0, snr_db=6.0, F=4, lead=300, tail=400):
    """F packets of random bits through a sparse channel plus white noise `snr_db` below the packet bodies' power.
    -> (r float64, starts int64 [F], bits [F * D * C * mu])."""
    from oracle import gf3_oracle as orc
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, size=F * p.D * p.C * p.mu)
    fill = p.const_points[rng.integers(0, len(p.const_points), size=p.K - p.C)]
    clean = orc.tx_stream(bits, fill, p, lead=lead, tail=tail)
    h = sparse_channel(rng, ntaps, decay)
    r = np.convolve(clean, h)[: len(clean)]
    starts = lead + np.arange(F) * p.frame_len + p.Lc
    body = np.concatenate([r[s: s + p.M * p.S] for s in starts])
    r = r + rng.standard_normal(len(r)) * np.sqrt(np.mean(body ** 2) / 10.0 ** (snr_db / 10.0))
    return r, starts, bits


def emulate(r, starts, p, tau=9.0):
    """The denoised path on the CPU: every pilot symbol of an applied row is overwritten by psum'/P (its prefix stays: the
    demodulator drops it), so that the oracle's mean over the pilot axis is the denoised estimate.
    -> (the stream to hand to oracle.demod_frames, report [F, 2, 5])."""
    out, rep, _, _ = denoise_frames(r, starts, p.N, p.CP, p.P, p.D, p.known_symbols(), tau)
    r2 = np.array(r, dtype=np.float64)
    for f, s in enumerate(starts):
        for side in range(2):
            if rep[f, side, 4]:
                for q in range(p.P):
                    at = s + (side * (p.P + p.D) + q) * p.S + p.CP
                    r2[at: at + p.N] = out[f, side] / p.P
    return r2, rep


def kernel_case(N, P, dtype, seed, D=2, snr_db=10.0):
    """The kernel test's input: three packets of 2P + D symbols, CP = N/16, carriers 10 .. 199, in the storage type `dtype`.
    Pilot symbols: the known symbol through a 24-tap channel plus noise; data symbols: noise.  Packet 0 holds a NaN in its
    second start pilot (float storage only: the integer types have none), packet 2 runs one sample past the stream.
    -> (p, x, starts)."""
    from oracle import gf3_oracle as orc
    rng = np.random.default_rng(seed)
    K = N // 2 - 1
    pts, bits = orc.qpsk_table()
    p = orc.RxParams(N=N, CP=N // 16, P=P, D=D, lo=10, hi=200, fit_lo=10, fit_hi=100, const_points=pts, const_bits=bits,
                     known_bits=rng.integers(0, 2, size=2 * K).astype(np.uint8))
    X = np.zeros(N // 2 + 1, dtype=complex)
    X[1:N // 2] = p.known_symbols()
    body = p.M * p.S
    starts = np.array([7, 7 + body + 33, 7 + 2 * body + 70])
    x = rng.standard_normal(starts[2] + body - 1)
    for f in range(3):
        clean = np.fft.irfft(X * np.fft.rfft(sparse_channel(rng, 24, 5.0), N), N)
        clean /= np.sqrt(np.mean(clean ** 2))
        sigma = 10.0 ** (-snr_db / 20.0)
        for q in list(range(P)) + list(range(P + D, 2 * P + D)):
            at = starts[f] + q * p.S
            sym = np.concatenate([clean[-p.CP:], clean]) + sigma * rng.standard_normal(p.S)
            x[at: at + p.S] = sym[: max(0, min(p.S, len(x) - at))]
    dtype = np.dtype(dtype)
    if dtype == np.int16:
        x = np.clip(np.rint(3000.0 * x), -32768, 32767).astype(dtype)
    elif dtype == np.uint8:
        x = np.clip(np.rint(128.0 + 20.0 * x), 0, 255).astype(dtype)
    else:
        x = x.astype(dtype)
        x[starts[0] + p.S + p.CP + 5] = np.nan
    return p, x, starts
