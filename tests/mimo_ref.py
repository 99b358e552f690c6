"""NumPy restatement of 2 x 2 spatial multiplexing ("Spatial multiplexing"; include/gf3rx.h), written from
the definition on top of the oracle (oracle/gf3_oracle.py), not from the kernels -- TEST INFRASTRUCTURE.

Wire format.  The encoded stream is cut into packets; packet 2q goes to speaker 0 and packet 2q + 1 to speaker 1,
sample-aligned.  Speaker 0 sends every chirp (the final one included), speaker 1 zeros for those samples.  In both pilot
blocks of speaker 1 the pilot symbols of odd index p (from the block's own first symbol) are negated, so at microphone b
    Y_p[k] = (H_b0[k] + (-1)^p H_b1[k]) X[k]     and, P being even,     cover t = mean_p (-1)^(t p) Y_p[k] / X[k] = H_bt[k].
One filler vector serves both speakers.

  tx_mimo(bits, fill, p)            -> the two speakers' streams [2, n]
  pilots(x, starts, p)              -> H [F, 2 sides, 2 covers, K], status [F]   (the means in ls_estimate's form)
  detect(Ys, Hs, slopes, p)         -> LLRs float32 [F, 2, D, C, mu] and the joint argmin's point indices [F, 2, D, C]
  receive_mimo(recordings, p, adv)  -> the whole chain on the oracle's sync, starts moved back by `adv` samples

and the scenario the tests share: a 2 x 2 channel of 40-tap decaying FIRs, speaker 1 arriving 6 samples early at
microphone 0 and 5 late at microphone 1 (`channel`, `through`, `add_noise`)."""
import numpy as np

from oracle import gf3_oracle as orc


# ---- transmit ----------------------------------------------------------------------------------------------------------
def cover(P):
    """[2 covers, P] signs: cover 0 all +1, cover 1 = (-1)^p"""
    if P < 2 or P % 2:
        raise ValueError("the pilot cover needs an even number of pilot symbols, at least 2")
    return np.stack([np.ones(P), (-1.0) ** np.arange(P)])


def tx_mimo(bits, fill_syms, p, lead=0, tail=2):
    """bits of an EVEN number of packets -> [2, n]: [lead zeros] + per pair [chirp | P pilots | D data | P pilots] +
    [final chirp] + [tail zeros]; speaker 1 with zeros under every chirp and the cover on its pilots."""
    rows = orc.tx_frames(bits, fill_syms, p)
    if rows.shape[0] % 2:
        raise ValueError("an even number of packets")
    first, second = rows[0::2], rows[1::2].copy()
    second[:, :p.Lc] = 0.0
    body = second[:, p.Lc:].reshape(second.shape[0], p.M, p.S)
    sign = cover(p.P)[1][None, :, None]
    body[:, :p.P] *= sign
    body[:, p.P + p.D:] *= sign
    s0 = np.concatenate([np.zeros(lead), first.reshape(-1), orc.chirp_replica(p), np.zeros(tail)])
    s1 = np.concatenate([np.zeros(lead), second.reshape(-1), np.zeros(p.Lc), np.zeros(tail)])
    return np.stack([s0, s1])


# ---- pilots ------------------------------------------------------------------------------------------------------------
def pilots(x, starts, p):
    """The two covers of both pilot blocks of every packet starting at starts[f] (first pilot sample, prefix included):
    cover t = (mean_p Re(s_tp Y_p) + i mean_p Im(s_tp Y_p)) / X, the order of oracle.ls_estimate.  A packet whose body
    leaves [0, len(x)) at either end: status 1 and NaN rows."""
    x = np.asarray(x, dtype=np.float64)
    F = len(starts)
    H = np.full((F, 2, 2, p.K), complex(np.nan, np.nan))
    status = np.zeros(F, dtype=np.int32)
    kn = p.known_symbols()
    car = np.arange(1, p.K + 1)
    sg = cover(p.P)
    L = p.M * p.S
    for f, s in enumerate(np.asarray(starts, dtype=np.int64)):
        if s < 0 or s + L > len(x):
            status[f] = 1
            continue
        X = np.fft.fft(x[s: s + L].reshape(p.M, p.S)[:, p.CP:])
        for side, blk in enumerate((X[:p.P, car], X[p.P + p.D:, car])):
            for t in range(2):
                v = blk * sg[t][:, None]
                H[f, side, t] = (v.real.mean(axis=0) + 1j * v.imag.mean(axis=0)) / kn
    return H, status


# ---- detector ----------------------------------------------------------------------------------------------------------
def channel_entries(H, slope, p):
    """One recording's H [F, 2, 2, K] and slope [F] -> h [2 columns][F, D, C] on the data carriers: the oracle's channel
    model of each column from its start and end estimate; the one slope serves both columns."""
    col = p.data_carriers - 1
    with np.errstate(invalid="ignore", over="ignore"):
        return [orc.channel_model(H[:, 0, t], H[:, 1, t], np.asarray(slope, dtype=np.float64), p)[:, :, col] for t in range(2)]


def sufficient(Ys, Hs, slopes, p):
    """-> (G00, G11, G01, m0, m1 [F, D, C], live [F, D, C]: any branch left): the sums over the branches, b ascending; a
    branch whose y or any of its four estimates at the cell is not finite is left out of all of them."""
    F = np.asarray(Hs[0]).shape[0]
    shape = (F, p.D, p.C)
    G00, G11 = np.zeros(shape), np.zeros(shape)
    G01, m0, m1 = (np.zeros(shape, dtype=complex) for _ in range(3))
    live = np.zeros(shape, dtype=bool)
    col = p.data_carriers - 1
    for Y, H, slope in zip(Ys, Hs, slopes):
        H = np.asarray(H, dtype=complex)
        y = np.asarray(Y, dtype=complex).reshape(F, p.D, p.N // 2 + 1)[:, :, p.data_carriers]
        h0, h1 = channel_entries(H, slope, p)
        fin = np.isfinite(H.real) & np.isfinite(H.imag)
        ok = (fin.all(axis=(1, 2))[:, None, col] & np.isfinite(y.real) & np.isfinite(y.imag)
              & np.isfinite(h0.real) & np.isfinite(h0.imag) & np.isfinite(h1.real) & np.isfinite(h1.imag))
        z = lambda v: np.where(ok, v, 0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            G00 = G00 + z(np.abs(h0) ** 2)
            G11 = G11 + z(np.abs(h1) ** 2)
            G01 = G01 + z(np.conj(h0) * h1)
            m0 = m0 + z(np.conj(h0) * y)
            m1 = m1 + z(np.conj(h1) * y)
        live |= ok
    return G00, G11, G01, m0, m1, live


def detect(Ys, Hs, slopes, p):
    """Joint max-log ML over the pairs (x0, x1) of table points:
        metric = G00 |x0|^2 + G11 |x1|^2 + 2 Re(conj(x0) G01 x1) - 2 Re(conj(x0) m0) - 2 Re(conj(x1) m1)
    LLR of a bit of stream s = min over the pairs with that bit 1 - min over the pairs with that bit 0; +0 where no branch
    is left.  -> (llr float32 [F, 2, D, C, mu], pair int64 [F, 2, D, C]: the table indices of the joint argmin)."""
    pts, lab = np.asarray(p.const_points), np.asarray(p.const_bits)
    M, mu = lab.shape
    G00, G11, G01, m0, m1, live = sufficient(Ys, Hs, slopes, p)
    e = lambda v: v[..., None, None]
    x0, x1 = pts[:, None], pts[None, :]                     # metric[..., i, j]: x0 = point i, x1 = point j
    metric = (e(G00) * np.abs(x0) ** 2 + e(G11) * np.abs(x1) ** 2 + 2.0 * (np.conj(x0) * e(G01) * x1).real
              - 2.0 * (np.conj(x0) * e(m0)).real - 2.0 * (np.conj(x1) * e(m1)).real)
    F = metric.shape[0]
    llr = np.zeros((F, 2, p.D, p.C, mu))
    for k in range(mu):
        one = lab[:, k] == 1
        llr[:, 0, :, :, k] = metric[..., one, :].min(axis=(-1, -2)) - metric[..., ~one, :].min(axis=(-1, -2))
        llr[:, 1, :, :, k] = metric[..., :, one].min(axis=(-1, -2)) - metric[..., :, ~one].min(axis=(-1, -2))
    llr = np.where(live[:, None, :, :, None], llr, 0.0)
    flat = metric.reshape(metric.shape[:-2] + (M * M,)).argmin(axis=-1)
    pair = np.stack([flat // M, flat % M], axis=1)
    return llr.astype(np.float32), pair


def zero_forcing(Ys, Hs, slopes, p):
    """What the detector is NOT: the per-carrier least-squares solve x = G^-1 m, each stream demapped on its own
    (max-log, scaled by its post-equalisation gain) -> llr float32 [F, 2, D, C, mu].  For the comparison of DESIGN §12."""
    pts, lab = np.asarray(p.const_points), np.asarray(p.const_bits)
    G00, G11, G01, m0, m1, _ = sufficient(Ys, Hs, slopes, p)
    det = G00 * G11 - np.abs(G01) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        xs = [(G11 * m0 - G01 * m1) / det, (G00 * m1 - np.conj(G01) * m0) / det]
        gains = [det / G11, det / G00]
    out = np.zeros(G00.shape[:1] + (2,) + G00.shape[1:] + (lab.shape[1],))
    for s in range(2):
        d2 = np.abs(xs[s][..., None] - pts) ** 2
        for k in range(lab.shape[1]):
            out[:, s, :, :, k] = (d2[..., lab[:, k] == 1].min(axis=-1) - d2[..., lab[:, k] == 0].min(axis=-1)) * gains[s]
    return np.nan_to_num(out).astype(np.float32)


def separation(Hs, p):
    """1 - |G01|^2 / (G00 G11) from the start-block estimates of the recordings' H [F, 2, 2, K] -> [F, C]"""
    col = p.data_carriers - 1
    h = np.stack([np.asarray(H)[:, 0] for H in Hs])[..., col]          # [B, F, 2, C]
    G00, G11 = (np.abs(h[:, :, 0]) ** 2).sum(axis=0), (np.abs(h[:, :, 1]) ** 2).sum(axis=0)
    G01 = (np.conj(h[:, :, 0]) * h[:, :, 1]).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1.0 - np.abs(G01) ** 2 / (G00 * G11)


# ---- the whole receive ---------------------------------------------------------------------------------------------------
def data_spectra(x, starts, p):
    """[F*D, N/2+1]: np.fft.rfft of every data symbol (prefix dropped) of the packets starting at starts[f]"""
    x = np.asarray(x, dtype=np.float64)
    rows = [x[s + (p.P + l) * p.S + p.CP: s + (p.P + l + 1) * p.S] for s in starts for l in range(p.D)]
    return np.fft.rfft(np.stack(rows))


def receive_mimo(recordings, p, advance=48):
    """Every recording: the oracle's own sync (it locks on speaker 0, which alone sends chirps); starts moved back by
    `advance`; the oracle's demodulation for the slope -- its Hs / He are cover 0 --; `pilots`; the data symbols' spectra.
    Then `detect`.  -> dict(llr [2F D C mu] in the coded order of packets 0, 1, 2, ..., bits, pair, starts [B, F] before
    the advance, H (per recording), slopes, separation [F, C])."""
    starts, Hs, slopes, Ys = [], [], [], []
    for r in recordings:
        st = orc.frame_starts(orc.chirp_method(r, p))
        starts.append(st)
        moved = st - advance
        slopes.append(orc.demod_frames(r, moved, p)["slope"])
        H, status = pilots(r, moved, p)
        if status.any():
            raise ValueError("a packet leaves the recording")
        Hs.append(H)
        Ys.append(data_spectra(r, moved, p))
    if len({len(s) for s in starts}) != 1:
        raise ValueError(f"the recordings hold different numbers of packets: {[len(s) for s in starts]}")
    llr, pair = detect(Ys, Hs, slopes, p)
    return dict(llr=llr.reshape(-1), bits=(llr.reshape(-1) < 0).astype(np.int64), pair=pair, starts=np.stack(starts), H=Hs,
                slopes=slopes, Y=Ys, separation=separation(Hs, p))


# ---- the scenario ------------------------------------------------------------------------------------------------------
TAPS = 40
LEAD = 8                    # samples every path is delayed by, so that an early arrival stays causal
SKEW = ((0, -6), (0, 5))    # SKEW[b][t]: arrival of speaker t at microphone b, in samples, relative to speaker 0 there
SEEDS = (20, 21, 22, 23)    # noise of microphone b


def channel(seed=1):
    """h[b][t]: 2 x 2 FIRs of TAPS taps, a unit first tap and a decaying random tail"""
    rng = np.random.default_rng(seed)
    h = np.zeros((2, 2, TAPS))
    h[:, :, 0] = 1.0
    h[:, :, 1:] = 0.8 * rng.normal(size=(2, 2, TAPS - 1)) * np.exp(-np.arange(1, TAPS) / 8.0)
    h[0, 1] *= 0.9
    h[1, 0] *= 0.8
    return h


def through(tx2, h=None):
    """The two speakers' streams [2, n] through the room -> [microphone 0, microphone 1] (noiseless, one length)"""
    h = channel() if h is None else h
    n = tx2.shape[1] + TAPS - 1 + LEAD + max(max(s) for s in SKEW)
    out = []
    for b in range(2):
        y = np.zeros(n)
        for t in range(2):
            at = LEAD + SKEW[b][t]
            seg = np.convolve(tx2[t], h[b][t])
            y[at: at + len(seg)] += seg
        out.append(y)
    return out


def add_noise(recordings, tx2, snr_db):
    """White Gaussian noise, seed SEEDS[b] at microphone b, snr_db below the RMS of a packet body as one speaker sends it
    (speaker 1's stream holds nothing else: its non-zero samples)"""
    body = np.asarray(tx2[1])[np.asarray(tx2[1]) != 0]
    sigma = np.sqrt(np.mean(body ** 2)) * 10.0 ** (-snr_db / 20.0)
    return [r + sigma * np.random.default_rng(s).normal(size=len(r)) for r, s in zip(recordings, SEEDS)]
