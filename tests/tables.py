"""A zoo of constellation tables and carrier maps, and the demodulation cases built from them (plain data and small
builders; nothing here touches a GPU).

Tables are `(points, bits)` in the oracle's format.  Each one is built to take one branch of the table classification of
`gf3_ctx_create` (`classify_table`, csrc/gf3rx_ctx.hip), named in the comment next to it; `classify` restates that
classification so that tests/test_tables_maps_cpu.py can check that every table lands where its comment says.

Carrier maps are functions K -> int array of 1-based FFT bins (K = N/2 - 1), in the order the output bits follow.  Only
`contig` is ascending and gap-free: every other map has `contig_lo == 0` in the library and goes through its `pos[]`
table."""
import functools

import numpy as np

from oracle import gf3_oracle as orc
from tests.util import load


def _bits_of(labels, mu):
    return ((np.asarray(labels)[:, None] >> np.arange(mu - 1, -1, -1)) & 1).astype(np.int64)


def _grid(lv_i, lv_q, lab_i, lab_q, bits_q):
    """Full grid: the label of (lv_i[a], lv_q[b]) is lab_i[a] in the leading bits, lab_q[b] in the last bits_q bits."""
    pts = np.array([complex(x, y) for x in lv_i for y in lv_q])
    labs = np.array([(a << bits_q) | b for a in lab_i for b in lab_q])
    mu = bits_q + int(np.ceil(np.log2(len(lv_i))))
    return pts, _bits_of(labs, mu)


GRAY4 = [0, 1, 3, 2]


def _tables():
    t = {}
    q_pts, q_bits = orc.qpsk_table()
    t["qpsk_ref"] = (q_pts, q_bits)                             # the reference's table: qpsk_q > 0, the sign kernel (control)
    order = [2, 0, 3, 1]
    t["qpsk_reordered"] = (q_pts[order], q_bits[order])          # same points and labels, rows in another order: qpsk_q = 0,
    #                                                              separable 2 x 2 uniform grid -> MODE_SCAN, grid fast path
    # natural-binary labels in the reference's row order (++ 00, +- 01, -- 10, -+ 11): the last bit is a function of
    # neither axis, so `sep` is refused although the points are a grid -> literal scan (NOT the grid path: a four-point
    # table takes that with `qpsk_reordered`)
    t["qpsk_relabelled"] = (q_pts, _bits_of([0, 1, 2, 3], 2))
    t["qpsk_rot"] = (np.array([1, 1j, -1, -1j], dtype=complex), _bits_of(GRAY4, 2))     # 3 x 3 levels for 4 points: no grid -> scan
    t["bpsk"] = (np.array([1, -1], dtype=complex), _bits_of([0, 1], 1))    # mu = 1; `sep` accepts (2 x 1), axis() refuses n = 1 -> scan
    # four equally spaced real levels, one Q level: `sep` accepts (4 x 1), axis() refuses the one-level axis -> scan
    t["pam4x1"] = (np.array([0.2, 0.6, 1.0, 1.4], dtype=complex), _bits_of(GRAY4, 2))
    lv4 = np.array([-3.0, -1.0, 1.0, 3.0])
    t["rect8"] = _grid(lv4 / np.sqrt(6), np.array([-1.0, 1.0]) / np.sqrt(6), GRAY4, [0, 1], 1)     # uniform grid, nI = 4 != nQ = 2, mu = 3
    # uniform grid whose axes differ in spacing and offset: loI != loQ, invI != invQ, lo != -hi on the I axis
    t["qam16_scaled_axes"] = _grid(0.4 * lv4 + 0.3, 0.2 * lv4, GRAY4, GRAY4, 2)
    lvu = 0.3 * np.array([-3.0, -1.0, 1.0, 4.0])
    t["qam16_unequal"] = _grid(lvu, lvu, GRAY4, GRAY4, 2)        # separable, unequal level spacing: `sep` accepted, `ug` refused -> scan
    p16, p16_bits = orc.square_qam_table(4)
    t["qam16_nonsep"] = (p16, _bits_of(np.random.RandomState(16).permutation(16), 4))     # grid points, labels of no axis -> scan
    t["psk8"] = (np.exp(2j * np.pi * np.arange(8) / 8), _bits_of(np.arange(8) ^ (np.arange(8) >> 1), 3))      # no grid -> scan, mu = 3
    t["ring8"] = (np.exp(2j * np.pi * (np.arange(8) + 0.25) / 8) * (1.0 + 0.3 * (np.arange(8) % 2)), _bits_of(np.arange(8), 3))   # two rings -> scan
    lv6 = np.arange(-5.0, 6.0, 2.0)
    cross = np.array([complex(x, y) for x in lv6 for y in lv6 if not (abs(x) == 5 and abs(y) == 5)]) / np.sqrt(20.0)
    t["cross32"] = (cross, _bits_of(np.arange(32), 5))           # 6 x 6 levels for 32 points: no full grid -> scan, mu = 5
    t["qam64"] = orc.square_qam_table(6)                         # uniform 8 x 8 grid (control)
    # 3 points on mu = 2 bits (M < 2^mu; label 10 is carried by no point): scan.  Used for hard decisions and transmit
    # only: it is kept out of the soft-decision tests (SOFT_TABLES).  (Any three distinct 2-bit labels show both values
    # of both bits, so the oracle's max-log formula has no empty set here; the exclusion is one of scope, not of need.)
    t["tri3"] = (np.array([1.0, np.exp(2j * np.pi / 3), np.exp(-2j * np.pi / 3)]), _bits_of([0, 1, 3], 2))
    # mu = 8, the widest label gf3_ctx_create accepts, on 16 points: the square 16-QAM with each 4-bit label repeated in both
    # nibbles.  Uniform grid -> per-axis fast path of the fused kernel with full 8-bit axis labels (0xcc / 0x33 masks);
    # hI + hQ = 4 != mu, so every soft path takes the literal "any table" emitter with all of its float[8] valid
    lab16 = (p16_bits * (1 << np.arange(3, -1, -1))).sum(axis=1)
    t["grid16_mu8"] = (p16, _bits_of(lab16 * 17, 8))
    # mu = 7 on ring8's points (no grid -> scan): labels (i << 4) | ((7 - i) << 1) | (i & 1), every bit takes both values
    i8 = np.arange(8)
    t["ring8_mu7"] = (t["ring8"][0], _bits_of((i8 << 4) | ((7 - i8) << 1) | (i8 & 1), 7))
    return t


TABLES = _tables()
SOFT_TABLES = [k for k in TABLES if k != "tri3"]
EXPECTED_CLASS = dict(qpsk_ref="qpsk", qpsk_reordered="uniform", qpsk_relabelled="scan", qpsk_rot="scan", bpsk="sep",
                      pam4x1="sep", rect8="uniform", qam16_scaled_axes="uniform", qam16_unequal="sep", qam16_nonsep="scan",
                      psk8="scan", ring8="scan", cross32="scan", qam64="uniform", tri3="scan", grid16_mu8="uniform",
                      ring8_mu7="scan")


def classify(points, bits):
    """The table classes of classify_table (csrc/gf3rx_ctx.hip), restated: 'qpsk' (the reference's table: sign kernel),
    'uniform' (separable grid, equally spaced levels on both axes: per-axis fast path in the fused kernel), 'sep' (separable
    grid only: the soft demapper's grid kernel; literal scan in the fused kernel), 'scan' (anything else)."""
    points, bits = np.asarray(points, dtype=complex), np.asarray(bits)
    M, mu = bits.shape
    lab = (bits * (1 << np.arange(mu - 1, -1, -1))).sum(axis=1)
    q = points[0].real
    if M == 4 and mu == 2 and 0.1 < q < 10 and np.array_equal(points, q * np.array([1 + 1j, 1 - 1j, -1 - 1j, -1 + 1j])) \
            and lab.tolist() == [0, 2, 3, 1]:
        return "qpsk"
    li, lq = list(dict.fromkeys(points.real)), list(dict.fromkeys(points.imag))
    if len(li) > 8 or len(lq) > 8 or len(li) * len(lq) != M or len({(z.real, z.imag) for z in points}) != M:
        return "scan"
    for b in range(mu):
        by_i = all(len(set(bits[points.real == x, b])) == 1 for x in li)
        by_q = all(len(set(bits[points.imag == y, b])) == 1 for y in lq)
        if not (by_i or by_q):
            return "scan"

    def uniform(lv):
        lv = np.sort(lv)
        if len(lv) < 2:
            return False
        step = (lv[-1] - lv[0]) / (len(lv) - 1)
        return bool(np.all(np.abs(lv - (lv[0] + np.arange(len(lv)) * step)) <= 1e-12 * step))
    return "uniform" if uniform(li) and uniform(lq) else "sep"


# ---- carrier maps: K -> 1-based bins, in output order -------------------------------------------------------------
def _band(K):
    return K // 5 + 1, K // 5 + 1 + K // 3


def contig(K):
    return np.arange(*_band(K))                                   # control: the only map with contig_lo > 0


def descending(K):
    return np.arange(*_band(K))[::-1].copy()                      # contiguous values, reversed order


def comb2(K):
    return np.arange(*_band(K))[::2].copy()


def comb3(K):
    return np.arange(1, K + 1, 3)


def two_bands(K):
    return np.concatenate([np.arange(K // 2, K // 2 + K // 5), np.arange(K // 8, K // 8 + K // 6)])    # upper band listed first


def shuffled(K):
    rs = np.random.RandomState(K)
    inner = rs.choice(np.arange(2, K), size=K // 3 - 2, replace=False)
    return rs.permutation(np.concatenate([[1, K], inner]))


def all_reversed(K):
    return np.arange(K, 0, -1)


def single_top(K):
    return np.array([K])


MAPS = dict(contig=contig, descending=descending, comb2=comb2, comb3=comb3, two_bands=two_bands, shuffled=shuffled,
            all_reversed=all_reversed, single_top=single_top)


# ---- parameter blocks and streams -----------------------------------------------------------------------------------
def params_for(table, N, carriers, P=2, D=3, CP=None):
    pts, bits = TABLES[table] if isinstance(table, str) else table
    K = N // 2 - 1
    mu = bits.shape[1]
    known = load("g6_realrec")["known_bits"]
    known = np.tile(known, -(-K * mu // len(known))).astype(np.uint8)
    if len(pts) < 1 << mu:                                         # pilots must not ask for a label that no point carries
        known = bits[np.random.RandomState(len(pts)).randint(0, len(pts), K)].reshape(-1).astype(np.uint8)
    return orc.RxParams(N=N, CP=N // 8 if CP is None else CP, P=P, D=D, carriers=np.asarray(carriers), const_points=pts,
                        const_bits=bits.astype(np.int64), known_bits=known, fit_lo=K // 8, fit_hi=K // 2)


def existing_labels_payload(rs, p, n_labels):
    """n_labels x mu random bits drawn from the labels the table carries (all of them unless M < 2^mu)."""
    return p.const_bits[rs.randint(0, len(p.const_points), n_labels)].reshape(-1)


QPSK_FILL = np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) / np.sqrt(2)
ECHO = np.zeros(40)
ECHO[[0, 3, 17, 39]] = 1.0, -0.35, 0.2, 0.08                      # echoes inside the prefix (test_phase_slope_over_whole_band)


def quantise(r, storage):
    """The samples as the given storage holds them (what both the engine and the oracle are then fed)."""
    if storage == "int16":
        return np.round(r / np.abs(r).max() * 30000).astype(np.int16)
    return r.astype(storage)


# One row per fused-demodulation case: table, map, N, P, D, F, sample storage.  Chosen so that every table meets a
# non-contiguous map, every map meets a uniform-grid table, a scan table and the reference's QPSK, and every N appears
# with a non-contiguous map (test_tables_maps_cpu.py asserts these rules and the geometries named in the comments).
CASES = [
    # table              map             N     P  D   F  storage
    ("qpsk_ref",          "contig",       1024, 2, 3,  2, "float64"),     # control
    ("qpsk_ref",          "descending",   1024, 2, 3,  2, "float64"),
    ("qpsk_ref",          "comb2",        2048, 1, 5,  2, "float64"),     # P = 1; C even: the QPSK packer's dword reads
    ("qpsk_ref",          "comb3",        4096, 2, 3,  2, "float32"),
    ("qpsk_ref",          "two_bands",    1024, 2, 4,  2, "float64"),
    ("qpsk_ref",          "shuffled",     8192, 2, 3,  2, "float64"),
    ("qpsk_ref",          "all_reversed", 1024, 2, 3,  3, "float64"),     # C = K odd: the generic packer on QPSK; D C mu = 3066
    ("qpsk_ref",          "single_top",   2048, 2, 70, 2, "float64"),     # C = 1: 16 symbols per word; two-phase: >= 2 chunks
    ("qam64",             "contig",       1024, 2, 3,  2, "float64"),     # control
    ("qam64",             "descending",   2048, 2, 3,  2, "float64"),
    ("qam64",             "shuffled",     4096, 2, 3,  2, "int16"),
    ("rect8",             "comb2",        1024, 2, 3,  2, "float64"),
    ("rect8",             "all_reversed", 2048, 2, 1,  3, "float64"),     # D = 1; C mu = 3 K odd
    ("rect8",             "single_top",   1024, 1, 23, 2, "float64"),     # 3 bits per symbol, labels straddle words; D C mu = 69
    ("qam16_scaled_axes", "two_bands",    4096, 2, 3,  2, "float64"),
    ("qam16_scaled_axes", "comb3",        1024, 2, 5,  2, "float64"),
    ("qpsk_reordered",    "comb3",        2048, 2, 3,  2, "float64"),
    ("qpsk_reordered",    "contig",       1024, 2, 3,  2, "float64"),
    ("qpsk_relabelled",   "descending",   1024, 2, 3,  2, "float64"),
    ("qpsk_rot",          "two_bands",    2048, 2, 3,  2, "float64"),
    ("bpsk",              "single_top",   1024, 2, 70, 2, "float64"),     # one bit per symbol: ring of 64 symbols; two-phase: 3 chunks
    ("bpsk",              "shuffled",     1024, 2, 5,  2, "float64"),     # C mu = 170, D C mu = 850: not a multiple of 8
    ("pam4x1",            "comb2",        1024, 2, 3,  2, "float64"),
    ("qam16_unequal",     "comb3",        8192, 2, 3,  2, "float32"),
    ("qam16_nonsep",      "all_reversed", 4096, 2, 3,  2, "float64"),
    ("psk8",              "contig",       2048, 2, 3,  2, "float64"),     # a scan table on the control map
    ("psk8",              "descending",   4096, 2, 40, 2, "float64"),     # two-phase: several chunks of a long packet
    ("psk8",              "all_reversed", 1024, 1, 5,  2, "float64"),     # C mu = 1533 odd, P = 1
    ("ring8",             "comb2",        8192, 2, 3,  2, "float64"),
    ("cross32",           "shuffled",     2048, 2, 3,  2, "float64"),     # mu = 5
    ("cross32",           "single_top",   4096, 2, 13, 2, "float64"),     # 5 bits per symbol, D C mu = 65
    ("tri3",              "two_bands",    1024, 2, 3,  2, "float64"),     # M < 2^mu
    # (appended: demod_case seeds by index, other files look rows up by index and id)
    ("grid16_mu8",        "shuffled",     1024, 2, 3,  2, "float64"),     # mu = 8: whole bytes per label
    ("grid16_mu8",        "two_bands",    4096, 2, 3,  2, "float32"),
    ("grid16_mu8",        "single_top",   1024, 2, 13, 2, "float64"),     # D C mu = 104: no multiple of 32 (of 8 it always is)
    ("ring8_mu7",         "comb2",        2048, 2, 3,  2, "float64"),     # mu = 7: labels straddle bytes and words
    ("ring8_mu7",         "all_reversed", 1024, 1, 3,  2, "float64"),     # C mu = 3577 odd, D C mu = 10731, P = 1
    ("ring8_mu7",         "single_top",   2048, 2, 13, 2, "float64"),     # D C mu = 91
]
CASE_IDS = [f"{t}-{m}-{N}-P{P}-D{D}-{st}" for t, m, N, P, D, F, st in CASES]
NOISE_REL = 0.01                                                   # white noise, fraction of the stream's rms
DRIFT = 3e-5                                                       # sampling-clock offset: the phase slope between a packet's two
#                                                                    pilot blocks that the channel model follows symbol by symbol


@functools.lru_cache(maxsize=None)
def demod_case(i):
    """Case i as (p, samples in their storage, starts, oracle output on those samples, payload bits).  The stream is the
    oracle transmitter's (random filler, random gaps) through the echo channel, resampled by 1 + DRIFT (so that the
    channel's phase turns from symbol to symbol and the fitted slope is far from zero), plus white noise, and every packet
    is started one sample late (a phase ramp over the band)."""
    table, mp, N, P, D, F, storage = CASES[i]
    K = N // 2 - 1
    p = params_for(table, N, MAPS[mp](K), P=P, D=D)
    rs = np.random.RandomState(1000 + i)
    payload = existing_labels_payload(rs, p, F * D * p.C)
    fill = rs.choice(QPSK_FILL, size=K - p.C)
    gaps = rs.randint(0, 200, F)
    lead = 30
    r = orc.tx_stream(payload, fill, p, gaps=gaps, lead=lead, tail=60)
    r = np.convolve(r, ECHO)[: len(r)]
    r = np.interp(np.arange(len(r)) * (1.0 + DRIFT), np.arange(len(r)), r)       # the receiver's clock runs slow
    r = r + NOISE_REL * np.sqrt(np.mean(r * r)) * rs.randn(len(r))
    true = lead + np.cumsum(gaps) + np.arange(F) * p.frame_len + p.Lc
    starts = np.round(true / (1.0 + DRIFT)).astype(np.int64) + 1
    x = quantise(r, storage)
    ref = orc.demod_frames(x.astype(np.float64), starts, p)
    return p, x, starts, ref, payload


def decision_gap(eq, points):
    """Smallest difference between the nearest and the second-nearest table distance over all symbols."""
    d = np.sort(np.abs(np.asarray(eq).reshape(-1, 1) - points), axis=1)
    return float((d[:, 1] - d[:, 0]).min())


NEAR_TIE_TABLES = ["psk8", "ring8", "cross32", "rect8", "qam16_unequal", "qam16_scaled_axes", "bpsk", "pam4x1", "grid16_mu8",
                   "ring8_mu7"]
# Tables on whose near-tie symbols a squared-distance argmin and the reference's argmin(abs(.)) differ somewhere.  For bpsk
# they cannot: its one boundary is Re = 0, and a symbol within a few ulp (of zero: denormals) or 1e-13 of it is at exactly
# the same rounded distance from +1 and -1 in either form, or on the same side in both.
NEAR_TIE_SQUARED_DIFFERS = set(NEAR_TIE_TABLES) - {"bpsk"}


def near_tie_symbols(points, seed):
    """Symbols on and within a few ulp of decision boundaries (the construction of
    test_demap_near_ties_match_the_reference_distance, for any table): mid-points of neighbouring points -- pairs no
    farther apart than 1.5 x the larger of their nearest-neighbour distances -- points along each such boundary, each
    shifted by 0, +-1, +-2, +-5 ulp on either axis and by 1e-13."""
    pts = np.asarray(points, dtype=complex)
    rs = np.random.RandomState(seed)
    i, j = np.triu_indices(len(pts), 1)
    d = np.abs(pts[i] - pts[j])
    full = np.abs(pts[:, None] - pts[None, :]) + np.diag(np.full(len(pts), np.inf))
    nn = full.min(axis=1)
    near = d <= 1.5 * np.maximum(nn[i], nn[j])
    mid = (pts[i[near]] + pts[j[near]]) / 2
    t = rs.uniform(-0.4, 0.4, size=(len(mid), 6)) * d[near][:, None]
    along = mid[:, None] + t * np.exp(1j * (np.angle(pts[i[near]] - pts[j[near]]) + np.pi / 2))[:, None]
    base = np.concatenate([mid, along.reshape(-1)])
    syms = [base]
    for k in (1, 2, 5):
        for ax in (0, 1):
            for sgn in (1, -1):
                re, im = base.real.copy(), base.imag.copy()
                for _ in range(k):
                    if ax == 0:
                        re = np.nextafter(re, sgn * np.inf)
                    else:
                        im = np.nextafter(im, sgn * np.inf)
                syms.append(re + 1j * im)
    syms.append(base + 1e-13)
    syms.append(base - 1e-13j)
    return np.concatenate(syms)


def squared_argmin_disagrees(sym, points):
    """Number of symbols on which argmin of dx^2 + dy^2 differs from the reference's argmin(abs(sym - table))."""
    d = np.abs(sym[:, None] - points[None, :])
    dx = sym.real[:, None] - points.real[None, :]
    dy = sym.imag[:, None] - points.imag[None, :]
    return int(((dx * dx + dy * dy).argmin(axis=1) != d.argmin(axis=1)).sum())
