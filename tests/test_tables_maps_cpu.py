"""The CPU half of tests/test_tables_maps_gpu.py: the zoo of tables and carrier maps (tests/tables.py) is built as its
comments say, the product of cases covers what it must, and every fused-demodulation case meets the condition under which
exact bit equality with the oracle is a fair demand.  No GPU is needed, so these run on every machine."""
import numpy as np
import pytest

from tests import tables as T


@pytest.mark.parametrize("name", list(T.TABLES))
def test_table_takes_the_branch_its_comment_names(name):
    pts, bits = T.TABLES[name]
    assert bits.shape == (len(pts), bits.shape[1]) and 2 <= len(pts) <= 64 and len(pts) <= 1 << bits.shape[1]
    lab = (bits * (1 << np.arange(bits.shape[1] - 1, -1, -1))).sum(axis=1)
    assert len(set(lab.tolist())) == len(pts) and len(set(pts.tolist())) == len(pts)      # one label per point, distinct points
    assert T.classify(pts, bits) == T.EXPECTED_CLASS[name]


@pytest.mark.parametrize("name", T.SOFT_TABLES)
def test_soft_tables_have_no_empty_set(name):
    """Every label bit takes both values over the table's points: the max-log formula has no empty set."""
    bits = T.TABLES[name][1]
    assert (bits.min(axis=0) == 0).all() and (bits.max(axis=0) == 1).all()


def test_the_widest_labels_are_in_the_zoo():
    """mu = 7 and mu = 8 (the widest gf3_ctx_create accepts) on tables of at most 64 points, in the soft tests too; the
    oracle's mapper and packer take them."""
    from oracle import gf3_oracle as orc
    assert {T.TABLES[n][1].shape[1] for n in T.SOFT_TABLES} >= {1, 2, 3, 4, 5, 6, 7, 8}
    for name, mu in (("grid16_mu8", 8), ("ring8_mu7", 7)):
        p = T.params_for(name, 1024, T.comb3(511), P=1, D=3)
        assert p.mu == mu and name in T.SOFT_TABLES
        payload = T.existing_labels_payload(np.random.RandomState(mu), p, p.D * p.C)
        X = orc.map_bits(payload.reshape(-1, p.C, p.mu), p)
        assert X.shape == (p.D, p.C) and np.isin(X, p.const_points).all()
        packed = orc.pack_bits(payload, p.D * p.C * p.mu)
        assert np.array_equal(np.unpackbits(packed.reshape(-1))[: payload.size], payload)


@pytest.mark.parametrize("K", [511, 1023, 2047, 4095])
def test_maps_are_what_they_claim(K):
    for name, fn in T.MAPS.items():
        m = fn(K)
        assert m.min() >= 1 and m.max() <= K and len(set(m.tolist())) == len(m), name
        is_contig = bool(np.array_equal(m, m[0] + np.arange(len(m))))
        assert is_contig == (name in ("contig", "single_top")), name        # (one bin is trivially a contiguous band)
    s = T.shuffled(K)
    assert 1 in s and K in s and abs(len(s) - K / 3) < 2 and not np.array_equal(s, np.sort(s))
    tb = T.two_bands(K)
    assert tb[0] > tb[-1] and len(np.unique(np.diff(np.sort(tb)))) == 2    # upper band first, one hole
    assert np.array_equal(T.all_reversed(K), np.arange(K, 0, -1)) and T.comb3(K)[0] == 1


def test_cases_cover_the_product_as_required():
    cls = {t: T.EXPECTED_CLASS[t] for t in T.TABLES}
    noncontig = lambda m: m != "contig"
    for t in T.TABLES:                                              # every table meets a non-contiguous map
        assert any(c[0] == t and noncontig(c[1]) for c in T.CASES), t
    for m in T.MAPS:                                                # every map meets a grid table, a scan table and reference QPSK
        met = {cls[c[0]] for c in T.CASES if c[1] == m}
        assert "uniform" in met and "qpsk" in met and ({"scan", "sep"} & met), (m, met)
    for N in (1024, 2048, 4096, 8192):                              # every N with a non-contiguous map
        assert any(c[2] == N and noncontig(c[1]) and c[1] != "single_top" for c in T.CASES), N
    geo = []
    for t, m, N, P, D, F, st in T.CASES:
        C, mu = len(T.MAPS[m](N // 2 - 1)), T.TABLES[t][1].shape[1]
        geo.append((C * mu, D * C * mu, D, P, st, noncontig(m)))
    assert any(b % 2 for b, *_ in geo)                              # C mu odd
    assert any(n % 8 for _, n, *_ in geo) and any(n % 32 and not n % 8 for _, n, *_ in geo)
    assert any(D == 1 for _, _, D, *_ in geo) and any(P == 1 for _, _, _, P, *_ in geo)
    assert {"float32", "int16"} <= {st for *_, st, nc in geo if nc}
    assert {32 % mu for mu in (T.TABLES[c[0]][1].shape[1] for c in T.CASES)} >= {0, 2}      # labels that straddle words (mu = 3, 5)
    for t, mu in (("ring8_mu7", 7), ("grid16_mu8", 8)):            # the widest labels: an odd C mu (mu = 7), one carrier alone
        rows = [c for c in T.CASES if c[0] == t]
        assert T.TABLES[t][1].shape[1] == mu and any(c[1] == "single_top" and (c[4] * mu) % 32 for c in rows), t
        assert any(c[1] == "single_top" and (c[4] * mu) % 8 for c in rows) == (mu == 7), t
        assert any((len(T.MAPS[c[1]](c[2] // 2 - 1)) * mu) % 2 for c in rows) == (mu == 7), t


@pytest.mark.parametrize("i", range(len(T.CASES)), ids=T.CASE_IDS)
def test_case_decisions_are_clear_of_every_boundary(i):
    """Exact bit equality between a kernel that equalises to 1e-9 x max(1, max|eq|) and the oracle is owed only where
    the oracle's own decision is not within that error of a boundary.  The gap between the nearest and the second-nearest
    table distance, over every data symbol of the case, must be at least 1e-7 x max(1, max|eq|): one hundred times the
    symbol tolerance.  No symbol is excluded."""
    p, x, starts, ref, payload = T.demod_case(i)
    assert ref["eq"].shape == (len(starts) * p.D, p.C) and np.isfinite(ref["eq"]).all()
    scale = max(1.0, float(np.abs(ref["eq"]).max()))
    gap = T.decision_gap(ref["eq"], p.const_points)
    print(f"{T.CASE_IDS[i]}: gap {gap:.3e}, max|eq| {scale:.3f}, BER {np.mean(ref['bits'] != payload):.2e}")
    assert gap >= 1e-7 * scale, (gap, scale)


@pytest.mark.parametrize("name", T.NEAR_TIE_TABLES)
def test_near_tie_symbols_are_not_vacuous(name):
    """Where rounding can make them differ at all, a squared-distance argmin disagrees with the reference's
    argmin(abs(.)) on some of the near-tie symbols: an engine that decided by squared distances alone would be caught."""
    pts = T.TABLES[name][0]
    sym = T.near_tie_symbols(pts, seed=len(name))
    n = T.squared_argmin_disagrees(sym, pts)
    print(name, len(sym), "symbols,", n, "where the squared-distance argmin differs")
    assert (n > 0) == (name in T.NEAR_TIE_SQUARED_DIFFERS), n
