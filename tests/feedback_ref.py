"""NumPy restatement of the decoder feedback (DESIGN §12, gf3_feedback_equalise and the loop of
CodedChain.decode_feedback), written from the definition, not from the kernel.

eq is [F*D, C] as demod_frames returns it (packet -> symbol -> carrier); `bits` and `known` hold F*D*C*mu bytes in
transmitted order (packet -> symbol -> carrier -> bit; non-zero = 1); `bins` are the context's data bins k_c.

  1. symbol (l, c) is known <=> all mu known bytes non-zero, eq[l, c] finite in both parts, some table entry's label equals
     its mu bits;  s = the FIRST such entry
  2. r = eq conj(s), q = |s|^2 on known symbols, 0 elsewhere
  3. W(l, c) = (l', c') of the same packet with |l' - l| <= half_symbols and |k_c' - k_c| <= half_bins
  4. A = sum_W r, B = sum_W q, n = known symbols in W                                           (fp64)
  5. g = A / B where n >= min_known and A != 0, else 1;  out = eq / g (eq itself where g = 1)
  6. S = sum_W |r| / B (0 where B = 0): the scale of the rounding error of A / B

The loop (`loop`): trusted = converged (and CRC matches, where a CRC is carried); trusted message rows are frozen; a pass
re-encodes them, masks their bits as known, runs steps 1-5 on the ORIGINAL eq, weighs the result and decodes the
untrusted codewords; it ends after `passes` passes, when nothing is untrusted, or when a pass trusts nothing new."""
import numpy as np

from tests import crc_ref as CR
from tests import ldpc_ref as R


def known_symbols(eq, bits, known, points, table_bits):
    """-> (ok [F*D, C] bool, s [F*D, C] complex: the first table entry of each symbol's label, 0 where there is none)"""
    eq = np.asarray(eq, dtype=np.complex128)
    tb = np.asarray(table_bits) != 0
    mu = tb.shape[1]
    b = (np.asarray(bits).reshape(eq.shape + (mu,)) != 0)
    kn = (np.asarray(known).reshape(eq.shape + (mu,)) != 0).all(axis=-1)
    idx = np.full(eq.shape, -1)
    for m in range(len(tb) - 1, -1, -1):                       # (descending: the first entry wins)
        idx = np.where((b == tb[m]).all(axis=-1), m, idx)
    ok = kn & np.isfinite(eq.real) & np.isfinite(eq.imag) & (idx >= 0)
    s = np.where(idx >= 0, np.asarray(points, dtype=np.complex128)[np.maximum(idx, 0)], 0.0)
    return ok, s


def feedback(eq, bits, known, points, table_bits, bins, D, half_symbols=2, half_bins=8, min_known=4):
    """-> (out, g, n, S), each [F*D, C].  The window sums are products with the two 0 / 1 membership matrices of step 3
    (symbols x symbols, carriers x carriers): every term of the definition once, nothing carried from window to window."""
    eq = np.asarray(eq, dtype=np.complex128)
    C = eq.shape[-1]
    F = eq.shape[0] // D
    k = np.asarray(bins, dtype=np.int64)
    assert eq.shape == (F * D, C) and k.shape == (C,)
    ok, s = known_symbols(eq, bits, known, points, table_bits)
    near = (np.abs(k[:, None] - k[None, :]) <= half_bins).astype(np.float64)          # [c', c]
    l = np.arange(D)
    rows = (np.abs(l[:, None] - l[None, :]) <= half_symbols).astype(np.float64)       # [l, l']

    def window(x):
        return np.einsum("lm,fmc->flc", rows, x.reshape(F, D, C) @ near).reshape(F * D, C)
    r = np.where(ok, eq, 0.0) * np.conj(s)
    A = window(r.real) + 1j * window(r.imag)
    B = window(np.where(ok, s.real ** 2 + s.imag ** 2, 0.0))
    M = window(np.abs(r))
    n = np.rint(window(ok.astype(np.float64))).astype(np.int64)
    use = (n >= min_known) & (A != 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        g = np.where(use, A / np.where(use, B, 1.0), 1.0 + 0.0j)
        out = np.where(g == 1, eq, eq / g)
        S = np.where(B > 0, M / np.where(B > 0, B, 1.0), 0.0)
    return out, g, n, S


def loop(eq, weigh, shifts, n_cw, points, table_bits, bins, D, passes, window=(2, 8), min_known=4, max_iter=50, crc=False,
         perm=None):
    """The feedback loop on eq [F*D, C].  weigh(eq) -> float32 LLRs in coded order (the interleaver undone);
    perm: None, or the per-packet map coded position i -> transmitted position perm[i] of the interleaver.
    -> dict(msg [n_cw, k]: the decoder's message rows, iters [n_cw], bad [n_cw] (CRC flags, zeros without one),
    trusted_in [n_cw]: the pass (0 = the first decode) that trusted each codeword, -1 for none, passes: passes run)."""
    sh = np.asarray(shifts)
    n = sh.shape[1] * R.Z
    eq = np.asarray(eq, dtype=np.complex128)
    mu = np.asarray(table_bits).shape[1]
    total = eq.size * mu
    F = eq.shape[0] // D
    per_packet = total // F

    def judge(msg, it):
        bad = CR.check(msg, msg.shape[1])[1] if crc else np.zeros(len(msg), dtype=np.uint8)
        return bad, (it > 0) & (bad == 0)

    llr = np.asarray(weigh(eq), dtype=np.float32)[: n_cw * n].reshape(n_cw, n)
    msg, _, iters = R.decode(sh, llr, max_iter)
    bad, trusted = judge(msg, iters)
    trusted_in = np.where(trusted, 0, -1)
    done = 0
    while done < passes and not trusted.all():
        coded = np.zeros(total, dtype=np.uint8)
        mask = np.zeros(total, dtype=np.uint8)
        coded[: n_cw * n] = (R.encode(sh, msg) * trusted[:, None]).reshape(-1)
        mask[: n_cw * n] = np.repeat(trusted.astype(np.uint8), n)
        if perm is not None:
            t_coded, t_mask = np.zeros_like(coded), np.zeros_like(mask)
            for f in range(F):
                t_coded[f * per_packet + perm] = coded[f * per_packet: (f + 1) * per_packet]
                t_mask[f * per_packet + perm] = mask[f * per_packet: (f + 1) * per_packet]
            coded, mask = t_coded, t_mask
        out = feedback(eq, coded, mask, points, table_bits, bins, D, window[0], window[1], min_known)[0]
        llr = np.asarray(weigh(out), dtype=np.float32)[: n_cw * n].reshape(n_cw, n)
        todo = np.flatnonzero(~trusted)
        m2, _, it2 = R.decode(sh, llr[todo], max_iter)
        msg[todo], iters[todo] = m2, it2
        b2, t2 = judge(m2, it2)
        bad[todo] = b2
        done += 1
        if not t2.any():
            break
        trusted[todo] = t2
        trusted_in[todo[t2]] = done
    return dict(msg=msg, iters=iters, bad=bad, trusted_in=trusted_in, passes=done)


def moving_echo(sig, first, S, D, P, alpha0, tau):
    """y[n] = x[n] + alpha_l x[n - tau]: an echo `tau` samples late (at most half the cyclic prefix) whose strength
    alpha_l = alpha0 sin^2(pi (l + 1/2) / D) holds over data symbol l's block of S samples (prefix included) and is 0 on the
    pilots, the chirp and the gaps.  `first`: the packet's body, i.e. the first pilot's cyclic prefix; data symbol l starts at
    first + (P + l) S."""
    x = np.asarray(sig, dtype=np.float64)
    alpha = np.zeros(len(x))
    a = alpha0 * np.sin(np.pi * (np.arange(D) + 0.5) / D) ** 2
    for l in range(D):
        alpha[first + (P + l) * S: first + (P + l + 1) * S] = a[l]
    late = np.concatenate([np.zeros(tau), x[: len(x) - tau]]) if tau else x
    return x + alpha * late
