"""Decoder feedback without a GPU: the NumPy restatement (tests/feedback_ref.py) on constructed cases, against a literal
loop over the definition; the coded chain's refusals; and the loop on a simplified channel model (no OFDM stage) with the
restated decoder: a moving echo that the two-point channel model cannot follow fails the codewords in the middle of a packet,
and feedback from the decoded ones recovers them."""
import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import feedback_ref as FB
from tests import ldpc_ref as R
from tests import noise_ref as NR
from tests import tables as T

QPSK = orc.qpsk_table()


def literal(eq, bits, known, table, bins, D, hs, hb, min_known):
    """The definition, symbol by symbol and term by term -> (g, n)."""
    pts, tb = table
    ok, s = FB.known_symbols(eq, bits, known, pts, tb)
    rows, C = eq.shape
    g = np.ones((rows, C), dtype=np.complex128)
    n = np.zeros((rows, C), dtype=np.int64)
    for i in range(rows):
        f, l = divmod(i, D)
        for c in range(C):
            A, B = 0.0 + 0.0j, 0.0
            for l2 in range(max(l - hs, 0), min(l + hs, D - 1) + 1):
                for c2 in range(C):
                    if abs(int(bins[c2]) - int(bins[c])) <= hb and ok[f * D + l2, c2]:
                        A += eq[f * D + l2, c2] * np.conj(s[f * D + l2, c2])
                        B += abs(s[f * D + l2, c2]) ** 2
                        n[i, c] += 1
            if n[i, c] >= min_known and A != 0:
                g[i, c] = A / B
    return g, n


def random_case(table, bins, F, D, density, seed, g0=0.8 - 0.3j, sigma=0.05):
    """Random points of the table times g0 plus noise, their labels as `bits`, a random symbol mask of `density`."""
    pts, tb = table
    rng = np.random.default_rng(seed)
    C, mu = len(bins), tb.shape[1]
    idx = rng.integers(0, len(pts), size=(F * D, C))
    eq = pts[idx] * g0 + sigma * (rng.normal(size=idx.shape) + 1j * rng.normal(size=idx.shape))
    bits = tb[idx].astype(np.uint8).reshape(-1)
    known = np.repeat((rng.random(size=(F * D, C)) < density).astype(np.uint8), mu)
    return eq, bits, known


def test_nothing_known_changes_nothing():
    bins = np.arange(10, 30)
    eq, bits, known = random_case(QPSK, bins, 2, 5, 0.0, 1)
    eq[3, 4] = complex(np.nan, 1.0)
    out, g, n, S = FB.feedback(eq, bits, known, *QPSK, bins, 5, 2, 8, 1)
    assert (g == 1).all() and not n.any() and not S.any()
    assert np.array_equal(out.view(np.float64), eq.view(np.float64), equal_nan=True)


def test_everything_known_recovers_the_gain_and_the_points():
    bins = np.arange(10, 30)
    g0 = 0.7 + 0.4j
    eq, bits, known = random_case(QPSK, bins, 2, 5, 1.0, 2, g0=g0, sigma=0.0)
    out, g, n, S = FB.feedback(eq, bits, known, *QPSK, bins, 5, 2, 3, 4)
    assert np.abs(g - g0).max() < 1e-14 and np.abs(out - eq / g0).max() < 1e-14
    assert n.max() == 5 * 7 and n.min() == 3 * 4                   # the full window, and a corner of the packet
    assert np.allclose(S, abs(g0), rtol=1e-14)
    assert np.array_equal(n, literal(eq, bits, known, QPSK, bins, 5, 2, 3, 4)[1])


def test_the_gate_counts_known_symbols():
    """Three known symbols side by side, then a fourth: with min_known = 4 the gain is used exactly where the window holds
    all four."""
    bins = np.arange(50, 70)
    D, mu = 6, 2
    eq, bits, _ = random_case(QPSK, bins, 1, D, 0.0, 3)
    mask = np.zeros((D, len(bins)), dtype=bool)
    mask[2, 5] = mask[2, 6] = mask[3, 5] = True
    known = np.repeat(mask.astype(np.uint8), mu)
    out, g, n, _ = FB.feedback(eq, bits, known, *QPSK, bins, D, 1, 2, 4)
    assert n.max() == 3 and (g == 1).all() and np.array_equal(out, eq)
    mask[3, 7] = True
    known = np.repeat(mask.astype(np.uint8), mu)
    out, g, n, _ = FB.feedback(eq, bits, known, *QPSK, bins, D, 1, 2, 4)
    four = np.zeros_like(mask)
    four[2:4, 5:8] = True                                          # rows 2..3 see rows 2 and 3; columns 5..7 see columns 5..7
    assert np.array_equal(n == 4, four) and np.array_equal(g != 1, four)
    gl, nl = literal(eq, bits, known, QPSK, bins, D, 1, 2, 4)
    assert np.array_equal(n, nl) and np.abs(g - gl).max() < 1e-14
    # one known byte of a symbol's mu cleared: the symbol is no longer known
    known[(3 * len(bins) + 7) * mu + 1] = 0
    assert FB.feedback(eq, bits, known, *QPSK, bins, D, 1, 2, 4)[2].max() == 3


def test_windows_stop_at_the_packet_edges():
    bins = np.arange(50, 60)
    D = 4
    eq, bits, _ = random_case(QPSK, bins, 2, D, 0.0, 4)
    mask = np.zeros((2 * D, len(bins)), dtype=bool)
    mask[D - 1] = True                                             # the last symbol of packet 0
    known = np.repeat(mask.astype(np.uint8), 2)
    out, g, n, _ = FB.feedback(eq, bits, known, *QPSK, bins, D, 2, 1, 1)
    assert not n[D:].any() and (g[D:] == 1).all() and np.array_equal(out[D:], eq[D:])
    assert n[: D - 3].max(initial=0) == 0 and n[D - 3: D].min() == 2 and n[D - 1, 4] == 3
    assert np.array_equal(n, literal(eq, bits, known, QPSK, bins, D, 2, 1, 1)[1])


@pytest.mark.parametrize("kind", ["shuffled", "descending", "comb3"])
def test_distance_is_measured_in_bins(kind):
    bins = T.MAPS[kind](63)
    D = 3
    eq, bits, known = random_case(T.TABLES["ring8"], bins, 2, D, 0.4, 5)
    table = T.TABLES["ring8"]
    out, g, n, S = FB.feedback(eq, bits, known, *table, bins, D, 1, 4, 3)
    gl, nl = literal(eq, bits, known, table, bins, D, 1, 4, 3)
    assert np.array_equal(n, nl) and np.abs(g - gl).max() <= 1e-13 * S.max()
    assert (g == 1).any() and (g != 1).any()
    assert np.abs(out - eq / gl).max() < 1e-12


def test_labels_no_point_carries_are_unknown_and_the_first_entry_wins():
    pts, tb = T.TABLES["tri3"]                                     # labels 00, 01, 11: 10 is carried by no point
    eq = np.full((1, 4), 0.5 + 0.5j)
    bits = np.array([0, 0, 1, 0, 1, 1, 0, 1], dtype=np.uint8)
    ok, s = FB.known_symbols(eq, bits, np.ones(8, np.uint8), pts, tb)
    assert ok.tolist() == [[True, False, True, True]] and np.array_equal(s[0, [0, 2, 3]], pts[[0, 2, 1]])
    twice = (np.array([1.0, -1.0, 1j]), np.array([[0], [1], [0]]))
    assert FB.known_symbols(eq[:, :1], [0], [1], *twice)[1][0, 0] == 1.0


def test_non_finite_symbols():
    bins = np.arange(10, 20)
    D = 3
    eq, bits, known = random_case(QPSK, bins, 1, D, 1.0, 6)
    base = FB.feedback(eq, bits, known, *QPSK, bins, D, 1, 1, 1)
    eq2 = eq.copy()
    eq2[1, 4] = complex(np.inf, 0.0)                               # at a known position: left out of the sums
    out, g, n, _ = FB.feedback(eq2, bits, known, *QPSK, bins, D, 1, 1, 1)
    assert n[1, 4] == base[2][1, 4] - 1 and np.isfinite(g.real).all() and np.isfinite(g.imag).all()
    assert not np.isfinite(out[1, 4].real) and np.isfinite(np.delete(out.reshape(-1), 14).real).all()
    assert np.array_equal(g[:, 7:], base[1][:, 7:])                # windows without it are untouched
    known2 = known.copy()
    known2[(1 * 10 + 4) * 2: (1 * 10 + 4) * 2 + 2] = 0              # at an unknown position: carried through
    out3, g3, n3, _ = FB.feedback(eq2, bits, known2, *QPSK, bins, D, 1, 1, 1)
    assert np.array_equal(n3, n) and np.array_equal(g3, g) and not np.isfinite(out3[1, 4].real)


# ---- the chain's refusals ---------------------------------------------------------------------------------------------
def chain(**kw):
    from gf3_audio_modem_amd.coding import CodedChain
    base = dict(encoding="QCLDPC-1/2", ldpc_n=1536, ldpc_max_iter=50, llr_weighting="csi", interleave=False, fused_llr=False,
                outer_code=None, per_packet=2800, make_code=lambda *a, **k: None)
    base.update(kw)
    return CodedChain(**base)


def test_the_chain_refuses_what_feedback_cannot_do():
    assert chain().check_receive() == ("1/2", False)
    assert chain().decoder_feedback == 0 and chain().feedback_window == (2, 8) and chain().feedback_min_known == 4
    assert chain(decoder_feedback=3).check_receive() == ("1/2", False)
    assert chain(decoder_feedback=3).feedback() == (3, 2, 8, 4)
    with pytest.raises(ValueError, match="decoder_feedback needs fused_llr = False"):
        chain(decoder_feedback=1, fused_llr=True).check_receive()
    assert chain(fused_llr=True).check_receive() == ("1/2", True)
    for enc in ("XOR", "None"):
        with pytest.raises(ValueError, match="decoder_feedback needs a 'QCLDPC-\\*' encoding"):
            chain(decoder_feedback=1, encoding=enc).check_receive()
        assert chain(encoding=enc).check_receive() == (None, False)
    for count in (-1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="decoder_feedback must be an integer >= 0"):
            chain(decoder_feedback=count).check_receive()
    for window in ((9, 8), (-1, 8), (2, 65), (2, -1), (2.0, 8), (2,), 3, (2, 8, 1)):
        with pytest.raises(ValueError, match="feedback.window"):
            chain(decoder_feedback=1, feedback_window=window).check_receive()
    for min_known in (0, -3, 1.5, None):
        with pytest.raises(ValueError, match="min_known"):
            chain(decoder_feedback=1, feedback_min_known=min_known).check_receive()
    assert chain(decoder_feedback=1, feedback_window=(0, 0), feedback_min_known=1).feedback() == (1, 0, 0, 1)
    assert chain(decoder_feedback=1, feedback_window=(8, 64)).feedback() == (1, 8, 64, 4)
    # off: the window is not looked at
    assert chain(feedback_window=(99, 99)).check_receive() == ("1/2", False)


def test_the_facade_carries_the_settings():
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2", encoding="QCLDPC-1/2")
    assert (rx.decoder_feedback, rx.feedback_window, rx.feedback_min_known) == (0, (2, 8), 4)
    rx.decoder_feedback, rx.feedback_window, rx.feedback_min_known = 2, (1, 4), 3
    c = rx._chain()
    assert (c.decoder_feedback, c.feedback_window, c.feedback_min_known) == (2, (1, 4), 3)


# ---- the loop on a simplified model -----------------------------------------------------------------------------------
def simulate(alpha, tau, sigma, seed, C=1400, D=24, passes=4):
    """eq = s g + noise on QPSK, g = 1 + alpha sin^2(pi (l + 1/2) / D) exp(-2 pi i k tau / 4096): a moving echo the pilots do not
    see.  Rate 1/2, one packet, 43 codewords, no interleaver, the project's restated noise weights.
    -> (the restated loop's result, the messages sent)"""
    from gf3_audio_modem_amd.ldpc import shift_table
    sh = shift_table("1/2")
    pts, tb = QPSK
    rng = np.random.default_rng(seed)
    bins = np.arange(100, 100 + C)
    n_cw = C * D * 2 // 1536
    msg = rng.integers(0, 2, size=(n_cw, 768), dtype=np.uint8)
    coded = rng.integers(0, 2, size=C * D * 2, dtype=np.uint8)    # (the fill past the last whole codeword)
    coded[: n_cw * 1536] = R.encode(sh, msg).reshape(-1)
    label = {tuple(b): p for p, b in zip(pts, tb)}
    s = np.array([label[tuple(b)] for b in coded.reshape(-1, 2)]).reshape(D, C)
    l = np.arange(D)[:, None]
    g = 1 + alpha * np.sin(np.pi * (l + 0.5) / D) ** 2 * np.exp(-2j * np.pi * bins[None, :] * tau / 4096)
    eq = s * g + sigma * (rng.normal(size=s.shape) + 1j * rng.normal(size=s.shape)) / np.sqrt(2)
    weigh = lambda e: NR.soft_demap_nw(e, NR.noise_estimate(e, pts, D), pts, tb, D)
    return FB.loop(eq, weigh, sh, n_cw, pts, tb, bins, D, passes), msg


def test_feedback_recovers_the_middle_of_a_packet_under_a_moving_echo():
    """alpha = 0.8, tau = 10, sigma = 0.35: the first decode leaves 5 of 43 codewords, one pass recovers them.  With the
    same seed and alpha = 0 every codeword decodes at once and no pass runs."""
    res, msg = simulate(0.8, 10, 0.35, 1)
    failed = np.flatnonzero(res["trusted_in"] != 0)
    print(f"first decode failed {failed.tolist()}, trusted in pass {res['trusted_in'][failed].tolist()}, passes {res['passes']}")
    assert len(failed) >= 3 and 10 < failed.min() and failed.max() < 33         # the middle of the packet
    assert 1 <= res["passes"] <= 4 and (res["trusted_in"] >= 0).all() and (res["iters"] > 0).all()
    assert np.array_equal(res["msg"], msg)
    res0, msg0 = simulate(0.0, 10, 0.35, 1)
    assert res0["passes"] == 0 and not res0["trusted_in"].any() and np.array_equal(res0["msg"], msg0)
    assert np.array_equal(msg0, msg)
