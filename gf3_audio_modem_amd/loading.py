"""Adaptive bit loading, host side (NumPy only): the per-carrier table of QAM orders, the rule that derives it from a
measured SNR, and the mapper of a loaded packet.  DESIGN §12.

A loading is `order`, uint8 [C] in data_carriers order, each entry 0, 2, 4 or 6 bits.  Bs = sum(order) coded bits
travel per data symbol, carrier c's at off[c] = sum(order[:c]); a packet carries D * Bs bits in the order packet ->
symbol -> carrier -> bit.  A carrier of order m > 0 uses engine.square_qam_table(m) (unit energy, label bits MSB first,
the first m/2 on the I axis) -- at m = 2 too, so an all-2 loading is NOT the reference's QPSK table, whose first bit
lies on the Q axis.  A carrier of order 0 carries no payload and transmits its bin's pilot symbol."""
import numpy as np

from .engine import map_bits, square_qam_table

ORDERS = (0, 2, 4, 6)


def validate_loading(order, C):
    """`order` as uint8 [C]; ValueError for a wrong length, a value outside {0, 2, 4, 6} or no loaded carrier."""
    a = np.asarray(order)
    if a.ndim != 1 or len(a) != C:
        raise ValueError(f"bit_loading must hold one order per data carrier ({C}), got shape {a.shape}")
    if not np.isin(a, ORDERS).all():
        bad = a[~np.isin(a, ORDERS)][0]
        raise ValueError(f"bit_loading: a carrier takes 0, 2, 4 or 6 bits, not {bad!r}")
    if not a.any():
        raise ValueError("bit_loading: no carrier is loaded")
    return np.ascontiguousarray(a, dtype=np.uint8)


def loading_layout(order):
    """(Bs, off): coded bits per data symbol and off [C + 1], off[c] the position of carrier c's first bit in its
    symbol's row (off[C] = Bs)."""
    off = np.concatenate([[0], np.cumsum(np.asarray(order, dtype=np.int64))])
    return int(off[-1]), off


def bit_loading_from_snr(snr_db, gap_db, max_bits=6):
    """The SNR-gap rule: order[c] is the largest b in (0, 2, 4, 6) with b <= max_bits and
    10 ** ((snr[c] - gap_db) / 10) >= 2 ** b - 1, stated in the linear domain so that no logarithm decides a boundary.
    snr_db is [C], or [F, C] (the receiver's last_snr_db): then each carrier's minimum over the packets counts.  A
    non-finite entry gives 0 bits.  -> uint8 [C].

    gap_db has no default: the gap of this project's codes under max-log demapping has not been measured.  The textbook
    8.8 dB (uncoded QAM at a symbol error rate of 1e-6) is the conservative end; a coded link takes less.  To measure the
    raw bit error rate of a choice, receive with encoding "None" under the loading: receive() then returns the hard
    decisions of the loaded carriers."""
    snr = np.asarray(snr_db, dtype=np.float64)
    if snr.ndim == 2:
        finite = np.isfinite(snr).all(axis=0)
        with np.errstate(invalid="ignore"):
            snr = np.where(finite, np.where(np.isfinite(snr), snr, 0.0).min(axis=0), np.nan)
    elif snr.ndim != 1:
        raise ValueError("snr_db must be [C] or [F, C]")
    ok = np.isfinite(snr)
    with np.errstate(over="ignore"):
        lin = np.where(ok, 10.0 ** ((np.where(ok, snr, 0.0) - float(gap_db)) / 10.0), 0.0)
    order = np.zeros(len(snr), dtype=np.uint8)
    for b in ORDERS[1:]:
        if b <= max_bits:
            order[ok & (lin >= 2.0 ** b - 1.0)] = b
    return order


def map_loaded(bits, order, known_symbols):
    """The loaded mapper: bits (n_sym * Bs of them, packet -> symbol -> carrier -> bit) -> complex [n_sym, C].
    known_symbols [C]: the pilot symbol of each data carrier's bin, which a carrier of order 0 transmits."""
    order = np.asarray(order)
    Bs, off = loading_layout(order)
    bits = np.asarray(bits).reshape(-1, Bs)
    out = np.empty((len(bits), len(order)), dtype=np.complex128)
    zero = order == 0
    out[:, zero] = np.asarray(known_symbols, dtype=np.complex128)[zero]
    for m in ORDERS[1:]:
        cs = np.flatnonzero(order == m)
        if len(cs):
            pts, lab = square_qam_table(m)
            idx = off[cs][:, None] + np.arange(m)                       # [n_c, m] bit positions in a row
            out[:, cs] = map_bits(bits[:, idx], pts, lab)
    return out
