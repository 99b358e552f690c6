"""The outer Reed-Solomon erasure code without a GPU: the NumPy restatement (tests/outer_ref.py) recovers what the code
promises and refuses what it cannot, and the façade's layout arithmetic (groups strided over the stream) holds."""
import itertools

import numpy as np
import pytest

from tests import outer_ref as O

ERASED, GOOD = -50, 3                                       # iteration counts as gf3_ldpc_decode reports them


def group(G, R, k, seed):
    """One group in transmitted order with NG = 1: [G + R, k] bits."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2, size=(G, k), dtype=np.uint8)
    return np.concatenate([data, O.encode(data, G, R)])


def erase(bits, members, seed):
    """Garbage in the erased rows, iters < 0 for them."""
    rng = np.random.default_rng(seed)
    out = bits.copy()
    iters = np.full(len(bits), GOOD, dtype=np.int32)
    for t in members:
        out[t] = rng.integers(0, 2, size=bits.shape[1], dtype=np.uint8)
        iters[t] = ERASED
    return out, iters


def test_field_and_cauchy_matrix():
    a = np.arange(256, dtype=np.uint8)
    assert np.array_equal(O.mul(a, np.uint8(1)), a) and not O.mul(a, np.uint8(0)).any()
    assert np.array_equal(O.mul(a, np.uint8(2))[128:130], [0x1D, 0x1F])            # x * x^7 = x^4 + x^3 + x^2 + 1
    for v in range(1, 256):
        assert O.mul(np.uint8(v), np.uint8(O.inv(v))) == 1
    C = O.cauchy(5, 3)
    assert C.shape == (3, 5) and C[1, 2] == O.inv(1 ^ (3 + 2)) and C.all()
    A = C[:, [0, 2, 4]]
    I = O.matvec(O.invert(A), A)
    assert np.array_equal(I, np.eye(3, dtype=np.uint8))


@pytest.mark.parametrize("G,R", [(2, 1), (3, 2), (5, 3)])
def test_every_pattern_of_at_most_r_erasures_is_recovered(G, R):
    bits = group(G, R, 24, seed=G)
    n = G + R
    for e in range(R + 1):
        for members in itertools.combinations(range(n), e):
            rx, iters = erase(bits, members, seed=e)
            got, status = O.recover(rx, iters, G, R)
            e_d = sum(t < G for t in members)
            assert status[0] == e_d, (members, status)
            assert np.array_equal(got[:G], bits[:G]), members               # the data is back
            assert np.array_equal(got[G:], rx[G:]), members                 # parity rows are never rewritten
            if e_d == 0:
                assert np.array_equal(got, rx)


@pytest.mark.parametrize("G,R,k", [(20, 4, 768), (239, 16, 40)])
def test_random_patterns(G, R, k):
    bits = group(G, R, k, seed=R)
    rng = np.random.default_rng(G)
    for trial in range(12):
        e = int(rng.integers(1, R + 1))
        members = rng.choice(G + R, size=e, replace=False)
        rx, iters = erase(bits, members, seed=trial)
        got, status = O.recover(rx, iters, G, R)
        assert status[0] == (members < G).sum()
        assert np.array_equal(got[:G], bits[:G])


@pytest.mark.parametrize("G,R", [(3, 2), (5, 3), (20, 4)])
def test_too_many_erasures_leave_the_group_untouched(G, R):
    bits = group(G, R, 32, seed=1)
    rx, iters = erase(bits, range(R + 1), seed=2)                            # R + 1 data members
    got, status = O.recover(rx, iters, G, R)
    assert status[0] == -(R + 1) and np.array_equal(got, rx)
    rx, iters = erase(bits, list(range(R)) + [G], seed=3)                    # R data members and one parity member
    got, status = O.recover(rx, iters, G, R)
    assert status[0] == -R and np.array_equal(got, rx)


def test_groups_of_one_call_are_independent():
    G, R, k, NG = 5, 3, 16, 4
    rng = np.random.default_rng(0)
    data = rng.integers(0, 2, size=(NG * G, k), dtype=np.uint8)
    par = O.encode(data, G, R)
    tx = np.concatenate([data.reshape(NG, G, k).transpose(1, 0, 2), par.reshape(NG, R, k).transpose(1, 0, 2)]).reshape(-1, k)
    iters = np.full(len(tx), GOOD, dtype=np.int32)
    rx = tx.copy()
    for g, members in enumerate([(), (0, 1, 2), (4, 5), (0, 1, 2, 3)]):
        for t in members:
            rx[t * NG + g] ^= 1
            iters[t * NG + g] = ERASED
    got, status = O.recover(rx, iters, G, R)
    assert status.tolist() == [0, 3, 1, -4]
    keep = np.ones(len(tx), dtype=bool)
    keep[[t * NG + 3 for t in range(4)]] = False                             # group 3 stays as it came
    keep[5 * NG + 2] = False                                                 # an erased parity row stays as it came
    assert np.array_equal(got[keep], tx[keep]) and np.array_equal(got[~keep], rx[~keep])


def test_refusals():
    for G, R, k in ((5, 0, 8), (5, 17, 8), (240, 16, 8), (5, 3, 12), (0, 1, 8)):
        with pytest.raises(ValueError):
            O.check_geometry(G, R, k)
    O.check_geometry(239, 16, 8)


# ---- the façade's layout -----------------------------------------------------------------------------------------
def test_layout_is_a_bijection_and_spreads_bursts():
    from gf3_audio_modem_amd import outer as P
    for per_packet, n, G, R in ((504000, 1536, 20, 4), (504000, 6144, 20, 4), (5000, 1536, 2, 1), (504000, 1536, 239, 16)):
        for F in (1, 2, 3, 7):
            cap, NG = P.layout(F, per_packet, n, G, R)
            assert (cap, NG) == (O.capacity(F, per_packet, n), O.groups(F, per_packet, n, G, R))
            assert cap == F * per_packet // n and NG == cap // (G + R) and NG * (G + R) <= cap
            if NG == 0:
                continue
            idx = np.array([[P.transmitted_index(g, t, NG) for t in range(G + R)] for g in range(NG)])
            assert sorted(idx.reshape(-1).tolist()) == list(range(NG * (G + R)))          # a bijection onto the first NG (G + R)
            group_of = np.empty(NG * (G + R), dtype=np.int64)
            group_of[idx] = np.arange(NG)[:, None]
            for start in range(0, NG * (G + R) - NG + 1, max(1, NG // 3)):                # any NG consecutive codewords
                assert len(set(group_of[start: start + NG].tolist())) == NG               # hit every group at most once


def test_smallest_packet_count():
    from gf3_audio_modem_amd import outer as P
    per_packet, n, k, G, R = 504000, 1536, 768, 20, 4
    for n_bits in (1, 199680, 199681, 399360, 399361, 10 ** 6):
        F = P.packets_for(n_bits, per_packet, n, k, G, R)
        assert F == O.packets_for(n_bits, per_packet, n, k, G, R)
        assert P.layout(F, per_packet, n, G, R)[1] * G * k >= n_bits
        assert F == 1 or P.layout(F - 1, per_packet, n, G, R)[1] * G * k < n_bits
        # the codewords of the groups end in the last packet: the coin-flip fill of encode() completes exactly F packets
        assert (F - 1) * per_packet < P.layout(F, per_packet, n, G, R)[1] * (G + R) * n <= F * per_packet or F == 1
    assert P.layout(1, 5000, 1536, 2, 1)[1] == 1 and P.layout(1, 4000, 1536, 2, 1)[1] == 0
    assert P.packets_for(10, 4000, 1536, 768, 2, 1) == 2                                   # NG(1) = 0: grow F


def test_geometry_of_the_impulse_scenario():
    """Mode A2, one packet, rate 1/2, n = 1536, (20, 4): the three clicked data symbols of tests/test_impulse_gpu.py cost
    every group at most one member, from the façade's own layout functions."""
    from gf3_audio_modem_amd.OFDM import receiver
    from gf3_audio_modem_amd import outer as P
    rx = receiver("A2", encoding="QCLDPC-1/2")
    assert rx.outer_code is None and rx.last_decode_report is None
    assert rx.outer_layout(1) == (328, 0)
    rx.outer_code = (20, 4)
    G, R = rx.outer_code
    per_packet = rx.packet_length * rx.data_bits_per_symbol
    assert per_packet == 504000 and rx.ldpc_n == 1536
    assert P.packets_for(150_000, per_packet, 1536, 768, G, R) == 1
    cap, NG = rx.outer_layout(1)
    assert (cap, NG) == (328, 13) and NG * G * 768 == 199_680 >= 150_000
    lo, hi = 70 * rx.data_bits_per_symbol, 73 * rx.data_bits_per_symbol       # data symbols 70 .. 72 in stream order
    assert (lo, hi) == (196_000, 204_400)
    hit = list(range(lo // 1536, (hi - 1) // 1536 + 1))
    assert hit == list(range(127, 134)) and len(hit) == 7 < NG
    assert max(hit) < NG * (G + R)
    groups = [cw % NG for cw in hit]                                          # codeword t NG + g belongs to group g
    assert all(P.transmitted_index(g, cw // NG, NG) == cw for g, cw in zip(groups, hit))
    assert len(set(groups)) == len(hit)                                       # at most one member per group <= R
    assert all(cw // NG < G for cw in hit)                                    # (all of them data members)
    bad = receiver("A2", encoding="XOR")
    bad.outer_code = (20, 4)
    with pytest.raises(ValueError, match="outer_code"):
        bad.encode(np.zeros(100, dtype=int))
    bad = receiver("A2", encoding="QCLDPC-1/2")
    bad.outer_code = 5
    with pytest.raises(ValueError, match="outer_code"):
        bad.outer_layout(1)
