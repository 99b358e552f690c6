"""NumPy restatement of the known-bit joint detector and of the cancellation loop built on it ("Cancelling
decoded streams"; gf3_mimo_detect_known, CodedChain.decode_cancel), written from the definition on top of tests/mimo_ref.py
and tests/ldpc_ref.py, not from the kernel -- TEST INFRASTRUCTURE.

`bits` and `known` hold F*2*D*C*mu bytes in the layout of the detector's LLRs [F, 2 streams, D, C, mu], which is the
transmitted order of packets 2f and 2f + 1; non-zero = 1 / known.

  detect_known(Ys, Hs, slopes, p, bits, known, w=None)     (llrs_known: the same before the rounding to float32)
      the plain scan of the 16 pairs (x0 = point i, x1 = point j) of mimo_ref.detect's metric.  A pair is admissible when,
      for both streams, every known bit of the cell equals that bit of the stream's point's label.  An unknown bit:
      min over the admissible pairs with it 1 - min over those with it 0, +0 where no branch is left.  A known bit:
      -LLR_KNOWN if it is 1, +LLR_KNOWN if it is 0, wherever it is.  w: joint_noise_ref's weights [B, F, C].
  loop(llr, redetect, shifts, n_cw, per_pair, passes, crc)
      trusted = converged (and the CRC matches, where one is carried); trusted message rows are frozen; a pass re-encodes
      them, marks their bits known, has `redetect` detect the packet pairs that hold a bit of an untrusted codeword again
      and decodes the untrusted codewords alone; it ends after `passes` passes, when nothing is untrusted, or when a pass
      trusts nothing new.
  receive(recordings, p, shifts, n_cw, passes, ...)   the whole chain on mimo_ref.receive_mimo's sync, estimates and spectra
  add_noise(recordings, tx2, snr_db, seeds)           mimo_ref.add_noise with the seeds as an argument"""
import numpy as np

from tests import crc_ref as CR
from tests import joint_noise_ref as JN
from tests import ldpc_ref as R
from tests import mimo_ref as MR

LLR_KNOWN = np.float32(1e30)


def metric(Ys, Hs, slopes, p):
    """-> (metric [F, D, C, i, j] of the pair (x0 = point i, x1 = point j), live [F, D, C])"""
    pts = np.asarray(p.const_points)
    G00, G11, G01, m0, m1, live = MR.sufficient(Ys, Hs, slopes, p)
    e = lambda v: v[..., None, None]
    x0, x1 = pts[:, None], pts[None, :]
    return (e(G00) * np.abs(x0) ** 2 + e(G11) * np.abs(x1) ** 2 + 2.0 * (np.conj(x0) * e(G01) * x1).real
            - 2.0 * (np.conj(x0) * e(m0)).real - 2.0 * (np.conj(x1) * e(m1)).real), live


def admissible(bits, known, lab):
    """bits, known [..., mu] bool of one stream's cells -> [..., M]: point m agrees with every known bit of the cell"""
    return (~known[..., None, :] | (bits[..., None, :] == (lab != 0))).all(axis=-1)


def detect_known(Ys, Hs, slopes, p, bits, known, w=None):
    """-> llr float32 [F, 2, D, C, mu]"""
    return llrs_known(Ys, Hs, slopes, p, bits, known, w).astype(np.float32)


def llrs_known(Ys, Hs, slopes, p, bits, known, w=None):
    """detect_known before the rounding to float32 -> float64 [F, 2, D, C, mu]"""
    if w is not None:
        Ys, Hs = JN.scaled(Ys, Hs, w, p)
    lab = np.asarray(p.const_bits)
    M, mu = lab.shape
    d, live = metric(Ys, Hs, slopes, p)
    F = d.shape[0]
    shape = (F, 2, p.D, p.C, mu)
    b = np.asarray(bits).reshape(shape) != 0
    k = np.asarray(known).reshape(shape) != 0
    ok = admissible(b[:, 0], k[:, 0], lab)[..., :, None] & admissible(b[:, 1], k[:, 1], lab)[..., None, :]
    d = np.where(ok, d, np.inf)
    llr = np.zeros(shape)
    with np.errstate(invalid="ignore"):
        for q in range(mu):
            one = lab[:, q] == 1
            llr[:, 0, :, :, q] = d[..., one, :].min(axis=(-1, -2)) - d[..., ~one, :].min(axis=(-1, -2))
            llr[:, 1, :, :, q] = d[..., :, one].min(axis=(-1, -2)) - d[..., :, ~one].min(axis=(-1, -2))
    llr = np.where(live[:, None, :, :, None], llr, 0.0)
    return np.where(k, np.where(b, -np.float64(LLR_KNOWN), np.float64(LLR_KNOWN)), llr)


def pairs_of(codewords, n, per_pair):
    """The packet pairs (ascending) that hold a bit of one of the codewords: codeword i is bits [i n, (i + 1) n)"""
    held = set()
    for i in np.asarray(codewords, dtype=np.int64):
        held.update(range(int(i * n // per_pair), int(((i + 1) * n - 1) // per_pair) + 1))
    return np.array(sorted(held), dtype=np.int64)


def loop(llr, redetect, shifts, n_cw, per_pair, passes, crc=False, max_iter=50):
    """llr: the first detection's LLRs in coded order (whole pairs).  redetect(pairs, bits [len(pairs), per_pair], known
    alike) -> those pairs' LLRs.  -> dict(msg [n_cw, k]: the decoder's message rows, iters [n_cw], bad [n_cw] (CRC flags,
    zeros without one), trusted_in [n_cw]: the pass (0 = the first decode) that trusted each codeword, -1 for none, passes:
    passes run, first: untrusted after the first decode, left: untrusted at the end)."""
    sh = np.asarray(shifts)
    n = sh.shape[1] * R.Z
    llr = np.array(llr, dtype=np.float32).reshape(-1)
    total = llr.size

    def judge(msg, it):
        bad = CR.check(msg, msg.shape[1])[1] if crc else np.zeros(len(msg), dtype=np.uint8)
        return bad, (it > 0) & (bad == 0)

    msg, _, iters = R.decode(sh, llr[: n_cw * n].reshape(n_cw, n), max_iter)
    bad, trusted = judge(msg, iters)
    trusted_in = np.where(trusted, 0, -1)
    first = int((~trusted).sum())
    done = 0
    while done < passes and not trusted.all():
        coded = np.zeros(total, dtype=np.uint8)
        mask = np.zeros(total, dtype=np.uint8)
        coded[: n_cw * n] = (R.encode(sh, msg) * trusted[:, None]).reshape(-1)
        mask[: n_cw * n] = np.repeat(trusted.astype(np.uint8), n)
        todo = np.flatnonzero(~trusted)
        pairs = pairs_of(todo, n, per_pair)
        llr.reshape(-1, per_pair)[pairs] = np.asarray(redetect(pairs, coded.reshape(-1, per_pair)[pairs],
                                                               mask.reshape(-1, per_pair)[pairs]), dtype=np.float32).reshape(len(pairs), per_pair)
        m2, _, it2 = R.decode(sh, llr[: n_cw * n].reshape(n_cw, n)[todo], max_iter)
        msg[todo], iters[todo] = m2, it2
        b2, t2 = judge(m2, it2)
        bad[todo] = b2
        done += 1
        if not t2.any():
            break
        trusted[todo] = t2
        trusted_in[todo[t2]] = done
    return dict(msg=msg, iters=iters, bad=bad, trusted_in=trusted_in, passes=done, first=first, left=int((~trusted).sum()))


def redetector(Ys, Hs, slopes, p, w=None):
    """`loop`'s redetect on the spectra, estimates and slopes of every packet pair (and the weights [B, F, C])"""
    NB = p.N // 2 + 1

    def redetect(pairs, bits, known):
        Yp = [np.asarray(Y).reshape(-1, p.D, NB)[pairs].reshape(-1, NB) for Y in Ys]
        wp = None if w is None else np.asarray(w)[:, pairs]
        return detect_known(Yp, [np.asarray(H)[pairs] for H in Hs], [np.asarray(s)[pairs] for s in slopes], p, bits, known, wp)
    return redetect


def receive(recordings, p, shifts, n_cw, passes, crc=False, advance=48, max_iter=50):
    """mimo_ref.receive_mimo, then `loop` on its LLRs -> (loop's dict, receive_mimo's dict)"""
    o = MR.receive_mimo(recordings, p, advance)
    per_pair = 2 * p.D * p.C * p.mu
    return loop(o["llr"], redetector(o["Y"], o["H"], o["slopes"], p), shifts, n_cw, per_pair, passes, crc, max_iter), o


def add_noise(recordings, tx2, snr_db, seeds=MR.SEEDS):
    """White Gaussian noise, seed seeds[b] at microphone b, snr_db below the RMS of a packet body as one speaker sends it"""
    body = np.asarray(tx2[1])[np.asarray(tx2[1]) != 0]
    sigma = np.sqrt(np.mean(body ** 2)) * 10.0 ** (-snr_db / 20.0)
    return [r + sigma * np.random.default_rng(s).normal(size=len(r)) for r, s in zip(recordings, seeds)]
