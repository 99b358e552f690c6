"""Deterministic cases for the coding kernels at the edges of what gf3_ldpc_create and the outer code accept
(tests/test_coding_shapes_cpu.py, tests/test_coding_shapes_gpu.py): shift tables by (mb, nb, Z, density, seed), their
LLRs, the special-value LLRs and the encoder shapes.  Everything is drawn from seeds; every reference is
tests/ldpc_ref_z.py, computed once per case and shared read-only.  Nothing here needs a GPU."""
import functools
import warnings

import numpy as np

from tests import ldpc_ref_z as RZ

MAX_ITER = 20                           # of every decoder case (the special-value cases: SPECIAL_MAX_ITER)
SPECIAL_MAX_ITER = 5
SIGMA_LADDER = (0.4, 1.4)               # BPSK noise levels of a case's codewords, first to last
N_LOAD = 4099                           # codewords of a launch "under load": odd, and at Z = 256 more than twice what
                                        # 256 compute units hold at six 24 KB workgroups each
# every read with one of these shifts crosses a wave boundary or wraps at Z = 256
WRAP_SHIFTS = (0, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255)
# the decoder kernel a code is dispatched to
REG, LDS, WIDE128, WIDE256 = "ldpc_decode_kernel<12>", "ldpc_decode_kernel<0>", "wide@128", "wide@256"


def kernel_of(mb, Z):
    """A copy of the dispatch at the end of gf3_ldpc_decode (csrc/gf3rx_ldpc.hip: Z > 64 -> the wide kernel, else
    mb <= 12 -> <12>, else <0>).  What test_coding_shapes_cpu.py says about "each of the four kernels" holds only while
    the two agree: a changed threshold there is changed here too."""
    return {128: WIDE128, 256: WIDE256}.get(Z) or (REG if mb <= 12 else LDS)


def shift_table(mb, nb, Z, density, seed, dual_diagonal=False, x=1, mid=1, shifts_from=None, row0_empty=False,
                full_row=None):
    """int16 [mb, nb] shift table.  A block is non-zero with probability `density` (1.0: every block), its shift drawn
    from [0, Z); every row has at least two non-zero blocks.  shifts_from: the drawn cells hold these values instead,
    laid out in turn (each of them as often as the others, to within one) and then permuted by the seed.  full_row:
    that row is non-zero in every column whatever the density.  dual_diagonal: the last mb columns are the
    dual-diagonal parity part with first-column shifts (x, 0, x) at rows 0, mid, mb-1 and only the nb - mb message
    columns are drawn; row0_empty leaves row 0 without a message block."""
    rng = np.random.default_rng(seed)
    pool = np.arange(Z) if shifts_from is None else np.asarray(shifts_from)
    cols = nb - mb if dual_diagonal else nb
    keep = rng.random((mb, cols)) < density
    if full_row is not None:
        keep[full_row] = True
    if shifts_from is None:
        draw = rng.choice(pool, (mb, cols))
    else:
        draw = rng.permutation(np.resize(pool, mb * cols)).reshape(mb, cols)
    sh = np.where(keep, draw, -1).astype(np.int16)
    if row0_empty:
        sh[0] = -1
    if dual_diagonal:
        assert mb >= 3 and 0 < mid < mb - 1 and 0 <= x < Z
        par = np.full((mb, mb), -1, dtype=np.int16)
        par[0, 0] = par[mb - 1, 0] = x
        par[mid, 0] = 0
        for c in range(1, mb):
            par[c - 1, c] = par[c, c] = 0
        sh = np.concatenate([sh, par], axis=1)
    else:
        for i in range(mb):
            short = 2 - int((sh[i] >= 0).sum())
            if short > 0:
                at = rng.choice(np.flatnonzero(sh[i] < 0), short, replace=False)
                sh[i, at] = rng.choice(pool, short)
    assert sh.shape == (mb, nb) and ((sh >= 0).sum(axis=1) >= 2).all() and sh.max() < Z
    assert (RZ.dual_diagonal(sh) is not None) == bool(dual_diagonal)
    return sh


def tiny_3x5_z64():
    """The 3 x 5 table of tests/test_ldpc_wide_gpu.py (tiny_z128) with its shifts reduced mod 64: dual-diagonal, x = 1."""
    t = np.array([[63, 64, 65, 0, -1], [65, 127, 0, 0, 0], [0, 64, 65, -1, 0]], dtype=np.int16)
    return np.where(t >= 0, t % 64, -1).astype(np.int16)


def codewords(sh, Z, n_cw, rng):
    """Codewords of the restated encoder for an encodable table, otherwise the all-zero codeword."""
    mb, nb = sh.shape
    if RZ.dual_diagonal(sh) is None:
        return np.zeros((n_cw, nb * Z), dtype=np.uint8)
    return RZ.encode(sh, rng.integers(0, 2, size=(n_cw, (nb - mb) * Z), dtype=np.uint8), Z)


def ladder_llrs(sh, Z, n_cw, seed, ladder=SIGMA_LADDER):
    """float32 [n_cw, n]: codewords over BPSK/AWGN, sigma on the ladder from the first to the last; the middle one
    carries exact zeros and exact magnitude ties (the plant of test_ldpc_wide_gpu.five_llrs, scaled down for short codes)."""
    assert 2 <= n_cw <= 12
    rng = np.random.default_rng(seed)
    cw = codewords(sh, Z, n_cw, rng)
    n = cw.shape[1]
    sig = np.linspace(*ladder, n_cw)[:, None]
    llr = ((1.0 - 2.0 * cw + rng.normal(size=cw.shape) * sig) * 2.0 / sig ** 2).astype(np.float32)
    c = n_cw // 2
    llr[c, rng.choice(n, min(40, n // 8), replace=False)] = 0.0
    t = rng.choice(n, min(60, n // 4), replace=False)
    llr[c, t[: len(t) // 2]] = 1.5
    llr[c, t[len(t) // 2:]] = -1.5
    llr[c] = np.round(llr[c])                              # many ties among the magnitudes (+-1.5 round to +-2)
    llr[c, t[: max(2, len(t) // 8)]] = 1.5
    return llr


# name -> (mb, nb, Z, density, codewords, options of shift_table)
_W = dict(shifts_from=WRAP_SHIFTS)
# One check of degree 32 repairs next to nothing: at sigma = 0.4 some of the 64 or 256 checks of such a code always
# stays unsatisfied, so its ladder starts where a whole codeword arrives without a wrong sign (sigma = 0.2).
LADDERS = {"1x32_z64": (0.2, 1.4), "1x32_z256": (0.2, 1.4)}
DECODER_CASES = {
    "1x2_z64": (1, 2, 64, 1.0, 12, {}),                    # degree 2, one layer
    "1x2_z128": (1, 2, 128, 1.0, 12, {}),
    "1x2_z256": (1, 2, 256, 1.0, 12, {}),
    "1x32_z64": (1, 32, 64, 1.0, 12, {}),                  # one row of degree 32
    "1x32_z256": (1, 32, 256, 1.0, 12, {}),
    "2x3_z128": (2, 3, 128, 1.0, 12, {}),
    "12x32_dense_z64": (12, 32, 64, 1.0, 12, {}),          # the largest register-state shape
    "12x32_dense_z256": (12, 32, 256, 1.0, 8, {}),         # 32 KB of LDS
    "12x32_sparse_z256": (12, 32, 256, 0.25, 12, {}),      # its converging companion
    "13x14_z64": (13, 14, 64, 0.5, 12, {}),                # the smallest LDS-state shape
    "13x32_z64": (13, 32, 64, 0.3, 12, {}),
    "31x32_dense_z64": (31, 32, 64, 1.0, 8, {}),           # the largest accepted shape, 39 KB of LDS
    "31x32_sparse_z64": (31, 32, 64, 0.2, 12, {}),
    "4x8_wrap_z256": (4, 8, 256, 1.0, 12, _W),             # every read crosses a wave boundary or wraps
    "4x8_wrap_dd_z256": (4, 8, 256, 1.0, 12, dict(_W, dual_diagonal=True, x=129, mid=2)),
    "3x5_z64": (3, 5, 64, None, 12, {}),                   # the register kernel on a custom encodable code
    # The codes above whose rows all have degree 32 stop after one iteration or never.  These keep ONE such row (row 3)
    # among sparse ones and converge in between: the stop rule taken after bit 31 of a sign word was really updated.
    "12x32_row32_z64": (12, 32, 64, 0.3, 12, dict(full_row=3)),
    "12x32_row32_z256": (12, 32, 256, 0.3, 12, dict(full_row=3)),
}
DEGREE_32_ROWS = ("1x32_z64", "1x32_z256", "12x32_dense_z64", "12x32_dense_z256", "31x32_dense_z64")
ONE_DEGREE_32_ROW = ("12x32_row32_z64", "12x32_row32_z256")
LOAD_CASES = ("family_r12_z64", "family_r12_z128", "family_r12_z256", "4x8_wrap_z256")
FAMILY_RATES = {"r12": "1/2"}
LOAD_CODEWORDS = 5


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def decoder_case(name):
    """(shift table, Z, LLRs [n_cw, n] read-only) of one decoder case; "family_r12_z<Z>" is the committed rate-1/2 code."""
    if name.startswith("family_"):
        from gf3_audio_modem_amd.ldpc import shift_table as family_table
        _, rate, z = name.split("_")
        Z = int(z[1:])
        sh, n_cw = family_table(FAMILY_RATES[rate], Z), LOAD_CODEWORDS
    else:
        mb, nb, Z, density, n_cw, opts = DECODER_CASES[name]
        sh = tiny_3x5_z64() if density is None else shift_table(mb, nb, Z, density, _seed(name), **opts)
        assert sh.shape == (mb, nb)
    if name in DEGREE_32_ROWS:
        assert (sh >= 0).all() and sh.shape[1] == 32       # every row has degree 32
    if name in ONE_DEGREE_32_ROW:
        assert ((sh >= 0).sum(axis=1) == 32).sum() == 1 and sh.shape[1] == 32
    llr = ladder_llrs(sh, Z, n_cw, _seed(name) + 1, LADDERS.get(name, SIGMA_LADDER))
    sh.setflags(write=False)
    llr.setflags(write=False)
    return sh, Z, llr


def _frozen(ref):
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def decoder_ref(name):
    """(bits, app, iters) of the restatement for decoder_case(name) at MAX_ITER; computed once, read-only."""
    sh, Z, llr = decoder_case(name)
    return _frozen(RZ.decode(sh, llr, MAX_ITER, Z))


def load_case(name):
    """LOAD_CODEWORDS codewords of a case, spread over its ladder, and their reference rows (a codeword's decoding does
    not depend on its neighbours in the launch): what is tiled to N_LOAD."""
    sh, Z, llr = decoder_case(name)
    rb, ra, ri = decoder_ref(name)
    pick = np.round(np.linspace(0, len(llr) - 1, LOAD_CODEWORDS)).astype(int)
    return sh, Z, llr[pick], (rb[pick], ra[pick], ri[pick])


# ---- special values ---------------------------------------------------------------------------------------------
SPECIAL_KINDS = ("plus_inf", "minus_inf", "both_inf", "nan", "near_flt_max", "subnormal", "minus_zero")
SPECIAL_CASES = {
    "4x8_z64": (4, 8, 64, 0.75),
    "4x8_z256": (4, 8, 256, 0.75),
    "13x14_z64": (13, 14, 64, 0.5),
}


def row_members(sh, Z, row, z):
    """Codeword positions of check row z of block row `row`, in column order."""
    return [j * Z + (z + s) % Z for j, s in RZ.rows_of(sh)[row]]


@functools.lru_cache(maxsize=None)
def special_case(name):
    """(shift table, Z, LLRs [7, n] read-only), one codeword per kind of SPECIAL_KINDS, each a moderately noisy all-zero
    codeword with the kind's values planted.  both_inf: -inf on the first and +inf on ALL other members of one check row
    (with two members only, a row of degree > 2 keeps a finite minimum, R stays finite and no inf - inf ever forms; with
    every member infinite R = +-inf, negative for the +inf members, and their APP = q + R is inf - inf in the first layer).  near_flt_max: +3e38 on every member
    of one check row (q + R = 3e38 + 2.25e38 overflows in the first layer) and +-3e38 alternating on those of another."""
    mb, nb, Z, density = SPECIAL_CASES[name]
    sh = shift_table(mb, nb, Z, density, _seed("special" + name))
    rng = np.random.default_rng(_seed(name) + 2)
    n = nb * Z
    llr = ((1.0 + rng.normal(size=(len(SPECIAL_KINDS), n)) * 0.7) * 2.0 / 0.7 ** 2).astype(np.float32)
    k = {kind: i for i, kind in enumerate(SPECIAL_KINDS)}
    llr[k["plus_inf"], rng.choice(n, 12, replace=False)] = np.inf
    llr[k["minus_inf"], rng.choice(n, 12, replace=False)] = -np.inf
    for e, p in enumerate(row_members(sh, Z, mb // 2, 5)):
        llr[k["both_inf"], p] = -np.inf if e == 0 else np.inf
    llr[k["nan"], rng.choice(n, 3, replace=False)] = np.nan
    for e, p in enumerate(row_members(sh, Z, mb - 1, Z - 1)):
        llr[k["near_flt_max"], p] = 3e38 if e % 2 == 0 else -3e38
    llr[k["near_flt_max"], row_members(sh, Z, 0, 7)] = 3e38
    llr[k["subnormal"]] = np.ldexp(llr[k["subnormal"]], -130)
    llr[k["minus_zero"], rng.choice(n, 40, replace=False)] = -0.0
    sh.setflags(write=False)
    llr.setflags(write=False)
    return sh, Z, llr


def quiet_decode(sh, llr, max_iter, Z):
    """The restatement with NumPy's invalid / overflow warnings silenced (inf - inf and 3e38 + 3e38 are the point)."""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return RZ.decode(sh, llr, max_iter, Z)


@functools.lru_cache(maxsize=None)
def special_ref(name, max_iter=SPECIAL_MAX_ITER):
    sh, Z, llr = special_case(name)
    return _frozen(quiet_decode(sh, llr, max_iter, Z))


# ---- encoder shapes ---------------------------------------------------------------------------------------------
# name -> (mb, nb, middle row, row 0 without message blocks); every one at each Z and each x of encoder_xs(Z)
ENCODER_SHAPES = {
    "3x4": (3, 4, 1, False),                               # mb = 3 is the minimum (middle row 1); one message column
    "3x32": (3, 32, 1, False),                             # 29 message columns
    "12x24_mid1": (12, 24, 1, False),
    "12x24_mid10": (12, 24, 10, False),
    "12x20_row0_empty": (12, 20, 5, True),                 # lambda_0 = 0
}


def encoder_xs(Z):
    return (0, 1, Z // 2, Z - 1)


@functools.lru_cache(maxsize=None)
def encoder_table(shape, Z, x):
    mb, nb, mid, row0_empty = ENCODER_SHAPES[shape]
    sh = shift_table(mb, nb, Z, 0.5, _seed(shape) + Z + x, dual_diagonal=True, x=x, mid=mid, row0_empty=row0_empty)
    assert RZ.dual_diagonal(sh) == (x, mid)
    if row0_empty:
        assert (sh[0, : nb - mb] < 0).all()
    sh.setflags(write=False)
    return sh


def messages(sh, Z, n_cw, seed):
    mb, nb = sh.shape
    return np.random.default_rng(seed).integers(0, 2, size=(n_cw, (nb - mb) * Z), dtype=np.uint8)


# ---- outer code -------------------------------------------------------------------------------------------------
# With (1, 1), (2, 1), (5, 3), (20, 4), (239, 16) of tests/test_outer_gpu.py: every RT in {1, 2, 4, 8, 16} of rs_dispatch
# at R = RT and, where there is one, at R < RT
OUTER_CODES = ((3, 2), (40, 2), (6, 5), (30, 7), (9, 8), (247, 8), (12, 9), (20, 13), (240, 15))
EVERY_ED_CODES = ((9, 8), (20, 13))     # recovery with every e_d in 1 .. R
# bytes per row (k / 8); a lane item is four of them, Q = ceil(bytes / 4)
LONG_ROWS = (1020, 1021, 1024, 1025, 2052)     # Q = 255, 256, 256, 257, 513: the 256-thread block, 2nd and 3rd trips
STEP_ROWS = (256, 260, 512, 516, 768)          # Q = 64, 65, 128, 129, 192: the other steps of the block-size rule
ROW_CODES = ((5, 3), (9, 8))
