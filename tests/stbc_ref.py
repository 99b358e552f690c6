"""NumPy restatement of transmit diversity -- two speakers, one microphone, the Alamouti space-time block code over pairs of
data symbols ("Transmit diversity"; include/gf3rx.h) -- written from the definition on top of the oracle
(oracle/gf3_oracle.py) and of tests/mimo_ref.py (cover, pilots, channel_entries, data_spectra, the scenario's room), not
from the kernels -- TEST INFRASTRUCTURE.

Wire format.  ONE encoded stream.  Chirps, pilots and cover are tx_mimo's: speaker 0 sends every chirp, speaker 1 zeros
for those samples and its pilot symbols of odd index negated.  With X_l the N-bin spectrum of data symbol l as the oracle's
tx_frames builds it (filler carriers included), for j = 0 .. D/2 - 1

    slot 2j:      speaker 0 sends  X_2j,             speaker 1  X_(2j+1)
    slot 2j + 1:  speaker 0 sends  -conj(X_(2j+1)),  speaker 1  conj(X_2j)

and, the symbols being real, conj(X) is the circular time reversal x[(-n) mod N] of the N-sample body under a prefix
rebuilt from the reversed body.  At microphone b, with a = 2j, b' = 2j + 1 and h_t(l) the channel entry of column t at
symbol l,   y_a = h0(a) x0 + h1(a) x1,   conj(y_b') = conj(h1(b')) x0 - conj(h0(b')) x1.

  tx_stbc(bits, fill, p)              -> the two speakers' streams [2, n]
  single_speaker / mono(bits, fill, p) -> the oracle's one stream on speaker 0 alone / on both speakers, [2, n]
  joint_slope(Hs, p)                  -> slope [F]: ONE fit on the product summed over recordings and columns
  detect(Ys, Hs, slope, p)            -> LLRs float32 [F, D, C, mu] and the joint argmin's point indices [F, D, C]
  receive_stbc(recordings, p, adv)    -> the whole chain on the oracle's sync, starts moved back by `adv` samples
  receive_single(recording, p, adv)   -> the oracle's own receive of one stream, starts moved back alike"""
import numpy as np

from oracle import gf3_oracle as orc
from tests import mimo_ref as MR


# ---- transmit ----------------------------------------------------------------------------------------------------------
def reversed_symbols(sym, p):
    """[..., S] symbols with their prefix -> the same with the body reversed in time, x[(-n) mod N], prefix rebuilt"""
    body = sym[..., p.CP:]
    rev = np.roll(body[..., ::-1], 1, axis=-1)
    return rev if p.CP == 0 else np.concatenate([rev[..., -p.CP:], rev], axis=-1)


def tx_stbc(bits, fill_syms, p, lead=0, tail=2):
    """bits of whole packets -> [2, n]: [lead zeros] + per packet [chirp | P pilots | D data | P pilots] + [final chirp] +
    [tail zeros]; speaker 1 with zeros under every chirp and the cover on its pilots; the data in Alamouti pairs."""
    if p.D % 2:
        raise ValueError("the code pairs the data symbols: an even number per packet")
    rows = orc.tx_frames(bits, fill_syms, p)
    F = rows.shape[0]
    first, second = rows.copy(), rows.copy()
    second[:, :p.Lc] = 0.0
    b0 = first[:, p.Lc:].reshape(F, p.M, p.S)                   # (views)
    b1 = second[:, p.Lc:].reshape(F, p.M, p.S)
    sign = MR.cover(p.P)[1][None, :, None]
    b1[:, :p.P] *= sign
    b1[:, p.P + p.D:] *= sign
    data = rows[:, p.Lc:].reshape(F, p.M, p.S)[:, p.P: p.P + p.D]
    even, odd = data[:, 0::2], data[:, 1::2]
    b0[:, p.P + 1: p.P + p.D: 2] = -reversed_symbols(odd, p)
    b1[:, p.P: p.P + p.D: 2] = odd
    b1[:, p.P + 1: p.P + p.D: 2] = reversed_symbols(even, p)
    s0 = np.concatenate([np.zeros(lead), first.reshape(-1), orc.chirp_replica(p), np.zeros(tail)])
    s1 = np.concatenate([np.zeros(lead), second.reshape(-1), np.zeros(p.Lc), np.zeros(tail)])
    return np.stack([s0, s1])


def single_speaker(bits, fill_syms, p, lead=0, tail=2):
    """The oracle's stream on speaker 0, speaker 1 switched off -> [2, n]"""
    s = orc.tx_stream(bits, fill_syms, p, lead=lead, tail=tail)
    return np.stack([s, np.zeros_like(s)])


def mono(bits, fill_syms, p, lead=0, tail=2):
    """The oracle's stream on both speakers -> [2, n]"""
    s = orc.tx_stream(bits, fill_syms, p, lead=lead, tail=tail)
    return np.stack([s, s])


# ---- the joint slope ---------------------------------------------------------------------------------------------------
def joint_product(Hs):
    """B arrays H [F, 2 sides, 2 covers, K] -> d [F, K] = sum_b sum_t conj(H_b[f, 0, t]) H_b[f, 1, t], b then t ascending"""
    d = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for H in Hs:
            H = np.asarray(H, dtype=complex)
            for t in range(2):
                d = d + np.conj(H[:, 0, t]) * H[:, 1, t]
    return d


def joint_slope(Hs, p):
    """The phase the channel gains per carrier between the two pilot blocks, fitted ONCE: y = unwrap(angle d) along the
    carriers, first-degree least squares over [fit_lo, fit_hi).  NaN for a packet with a non-finite d in the fit range."""
    d = joint_product(Hs)[:, p.fit_lo: p.fit_hi]
    if d.shape[1] < 2:
        raise ValueError("phase-slope fit range holds fewer than 2 carriers")
    out = np.full(d.shape[0], np.nan)
    x = np.arange(d.shape[1])
    for f in range(d.shape[0]):
        if np.isfinite(d[f].real).all() and np.isfinite(d[f].imag).all():
            out[f] = np.polyfit(x, np.unwrap(np.angle(d[f])), 1)[0]
    return out


# ---- detector ----------------------------------------------------------------------------------------------------------
def sufficient(Ys, Hs, slope, p):
    """-> (G00, G11, G01, m0, m1 [F, D/2, C], live [F, D/2, C]: any branch left): the sums over the branches, b ascending; a
    branch whose y at either slot of the pair, or any of whose four estimates at the carrier, or whose channel entry is not
    finite is left out of all of them."""
    F = np.asarray(Hs[0]).shape[0]
    shape = (F, p.D // 2, p.C)
    G00, G11 = np.zeros(shape), np.zeros(shape)
    G01, m0, m1 = (np.zeros(shape, dtype=complex) for _ in range(3))
    live = np.zeros(shape, dtype=bool)
    col = p.data_carriers - 1
    fin = lambda v: np.isfinite(v.real) & np.isfinite(v.imag)
    for Y, H in zip(Ys, Hs):
        H = np.asarray(H, dtype=complex)
        y = np.asarray(Y, dtype=complex).reshape(F, p.D, p.N // 2 + 1)[:, :, p.data_carriers]
        h0, h1 = MR.channel_entries(H, slope, p)
        ya, yb = y[:, 0::2], y[:, 1::2]
        h0a, h0b, h1a, h1b = h0[:, 0::2], h0[:, 1::2], h1[:, 0::2], h1[:, 1::2]
        ok = (fin(H).all(axis=(1, 2))[:, None, col] & fin(ya) & fin(yb) & fin(h0a) & fin(h0b) & fin(h1a) & fin(h1b))
        z = lambda v: np.where(ok, v, 0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            G00 = G00 + z(np.abs(h0a) ** 2 + np.abs(h1b) ** 2)
            G11 = G11 + z(np.abs(h1a) ** 2 + np.abs(h0b) ** 2)
            G01 = G01 + z(np.conj(h0a) * h1a - h1b * np.conj(h0b))
            m0 = m0 + z(np.conj(h0a) * ya + h1b * np.conj(yb))
            m1 = m1 + z(np.conj(h1a) * ya - h0b * np.conj(yb))
        live |= ok
    return G00, G11, G01, m0, m1, live


def detect(Ys, Hs, slope, p):
    """Joint max-log ML of every pair (x0 = symbol 2j, x1 = symbol 2j + 1) over the pairs of table points, mimo_ref.detect's
    metric on the statistics above:
        metric = G00 |x0|^2 + G11 |x1|^2 + 2 Re(conj(x0) G01 x1) - 2 Re(conj(x0) m0) - 2 Re(conj(x1) m1)
    -> (llr float32 [F, D, C, mu]; +0 where no branch is left,  pair int64 [F, D, C]: the table index of the joint argmin)."""
    pts, lab = np.asarray(p.const_points), np.asarray(p.const_bits)
    M, mu = lab.shape
    G00, G11, G01, m0, m1, live = sufficient(Ys, Hs, np.asarray(slope, dtype=np.float64), p)
    e = lambda v: v[..., None, None]
    x0, x1 = pts[:, None], pts[None, :]                     # metric[..., i, j]: x0 = point i, x1 = point j
    metric = (e(G00) * np.abs(x0) ** 2 + e(G11) * np.abs(x1) ** 2 + 2.0 * (np.conj(x0) * e(G01) * x1).real
              - 2.0 * (np.conj(x0) * e(m0)).real - 2.0 * (np.conj(x1) * e(m1)).real)
    F = metric.shape[0]
    llr = np.zeros((F, p.D, p.C, mu))
    for k in range(mu):
        one = lab[:, k] == 1
        llr[:, 0::2, :, k] = metric[..., one, :].min(axis=(-1, -2)) - metric[..., ~one, :].min(axis=(-1, -2))
        llr[:, 1::2, :, k] = metric[..., :, one].min(axis=(-1, -2)) - metric[..., :, ~one].min(axis=(-1, -2))
    llr = np.where(np.repeat(live, 2, axis=1)[..., None], llr, 0.0)
    flat = metric.reshape(metric.shape[:-2] + (M * M,)).argmin(axis=-1)
    pair = np.zeros((F, p.D, p.C), dtype=np.int64)
    pair[:, 0::2], pair[:, 1::2] = flat // M, flat % M
    return llr.astype(np.float32), pair


# ---- the whole receive ---------------------------------------------------------------------------------------------------
def receive_stbc(recordings, p, advance=48, slope="joint"):
    """Every recording: the oracle's own sync (it locks on speaker 0, which alone sends chirps); starts moved back by
    `advance`; `mimo_ref.pilots`; the data symbols' spectra.  Then ONE slope -- `joint_slope`, or with slope="reference" the
    oracle's own fit on recording 0's path from speaker 0 (what the feature does NOT do; for the comparison) -- and `detect`.
    -> dict(llr [F D C mu] flat, bits, pair, starts [B, F] before the advance, H (per recording), slope, Y, stats)."""
    starts, Hs, Ys = [], [], []
    for r in recordings:
        st = orc.frame_starts(orc.chirp_method(r, p))
        starts.append(st)
        moved = st - advance
        H, status = MR.pilots(r, moved, p)
        if status.any():
            raise ValueError("a packet leaves the recording")
        Hs.append(H)
        Ys.append(MR.data_spectra(r, moved, p))
    if len({len(s) for s in starts}) != 1:
        raise ValueError(f"the recordings hold different numbers of packets: {[len(s) for s in starts]}")
    sl = joint_slope(Hs, p) if slope == "joint" else orc.phase_slope(Hs[0][:, 0, 0], Hs[0][:, 1, 0], p)
    llr, pair = detect(Ys, Hs, sl, p)
    return dict(llr=llr.reshape(-1), bits=(llr.reshape(-1) < 0).astype(np.int64), pair=pair, starts=np.stack(starts), H=Hs,
                slope=sl, Y=Ys, stats=sufficient(Ys, Hs, sl, p))


def receive_single(r, p, advance=0):
    """The oracle's receive of ONE stream from one recording, every start moved back by `advance` -> its demod_frames dict"""
    st = orc.frame_starts(orc.chirp_method(r, p))
    out = orc.demod_frames(r, st - advance, p)
    out["starts"] = st
    return out


# ---- noise ---------------------------------------------------------------------------------------------------------------
def body_rms(tx2):
    """RMS of a packet body as ONE speaker sends it (speaker 1's stream holds nothing else: its non-zero samples)"""
    body = np.asarray(tx2[1])[np.asarray(tx2[1]) != 0]
    return np.sqrt(np.mean(body ** 2))


def add_noise(recordings, rms, snr_db, mics=None):
    """White Gaussian noise snr_db below `rms`, seed mimo_ref.SEEDS[b] at microphone b (mics: which microphone each is)"""
    sigma = rms * 10.0 ** (-snr_db / 20.0)
    mics = range(len(recordings)) if mics is None else mics
    return [r + sigma * np.random.default_rng(MR.SEEDS[b]).normal(size=len(r)) for r, b in zip(recordings, mics)]
