"""The inputs of tests/test_coding_shapes_gpu.py, judged from the restatements alone (no GPU): every decoder case takes
both stop rules, every decoder kernel has a case that stops in the middle, the special values do in the restatement what
they were planted for, the Z = 64 restatements agree on the custom codes, and the restated encoder's codewords satisfy
the expanded H.  Without these a GPU test could pass vacuously."""
import numpy as np
import pytest

from tests import coding_cases as CC
from tests import ldpc_ref as R64
from tests import ldpc_ref_z as RZ
from tests import outer_ref as O

ALL_DECODER_CASES = list(CC.DECODER_CASES) + [c for c in CC.LOAD_CASES if c not in CC.DECODER_CASES]
FLT_MIN_NORMAL = np.float32(2.0 ** -126)


def test_shift_tables_are_what_the_case_list_says():
    for name, (mb, nb, Z, density, n_cw, opts) in CC.DECODER_CASES.items():
        sh, z, llr = CC.decoder_case(name)
        assert z == Z and sh.shape == (mb, nb) and sh.dtype == np.int16 and llr.shape == (n_cw, nb * Z)
        assert sh.min() >= -1 and sh.max() < Z and ((sh >= 0).sum(axis=1) >= 2).all()
        assert 2 <= n_cw <= 12 and llr.dtype == np.float32 and np.isfinite(llr).all()
        mid = llr[n_cw // 2]
        assert (mid == 0).any() and (np.abs(mid) == 1.5).sum() >= 2           # the planted zeros and ties
        if density == 1.0:
            assert (sh[:, : nb - mb if opts.get("dual_diagonal") else nb] >= 0).all()
    for name in CC.DEGREE_32_ROWS:
        assert ((CC.decoder_case(name)[0] >= 0).sum(axis=1) == 32).all()
    for name in CC.ONE_DEGREE_32_ROW:                                         # one such row among sparse ones
        deg = (CC.decoder_case(name)[0] >= 0).sum(axis=1)
        assert (deg == 32).sum() == 1 and np.median(deg) <= 12, deg
    assert ((CC.decoder_case("1x2_z64")[0] >= 0).sum(axis=1) == 2).all()
    for name in ("4x8_wrap_z256", "4x8_wrap_dd_z256"):
        sh = CC.decoder_case(name)[0]
        body = sh[:, :4] if name.endswith("dd_z256") else sh
        assert set(body.ravel().tolist()) == set(CC.WRAP_SHIFTS)              # every one of them, and nothing else
        assert (RZ.dual_diagonal(sh) is not None) == name.endswith("dd_z256")
    assert RZ.dual_diagonal(CC.decoder_case("4x8_wrap_dd_z256")[0]) == (129, 2)
    assert RZ.dual_diagonal(CC.decoder_case("3x5_z64")[0]) == (1, 1)
    a, b = CC.shift_table(5, 9, 128, 0.4, 3), CC.shift_table(5, 9, 128, 0.4, 3)
    assert np.array_equal(a, b) and not np.array_equal(a, CC.shift_table(5, 9, 128, 0.4, 4))     # a function of the seed


@pytest.mark.parametrize("name", ALL_DECODER_CASES)
def test_every_decoder_case_takes_both_stop_rules(name):
    _, _, ri = CC.decoder_ref(name)
    assert (ri > 0).any() and (ri < 0).any(), ri
    assert ((ri == -CC.MAX_ITER) | ((ri >= 1) & (ri <= CC.MAX_ITER))).all()


def test_every_decoder_kernel_stops_in_the_middle_somewhere():
    seen = {}
    for name in ALL_DECODER_CASES:
        sh, Z, _ = CC.decoder_case(name)
        ri = CC.decoder_ref(name)[2]
        if ((ri > 1) & (ri < CC.MAX_ITER)).any():
            seen.setdefault(CC.kernel_of(sh.shape[0], Z), []).append(name)
    assert set(seen) == {CC.REG, CC.LDS, CC.WIDE128, CC.WIDE256}, seen
    # the custom shapes alone do it too, the family codes aside
    custom = {k: [n for n in v if not n.startswith("family_")] for k, v in seen.items()}
    assert all(custom.values()), custom
    # every kernel also has a case at its extreme shape
    kernels = {name: CC.kernel_of(CC.DECODER_CASES[name][0], CC.DECODER_CASES[name][2]) for name in CC.DECODER_CASES}
    assert kernels["31x32_dense_z64"] == kernels["13x14_z64"] == CC.LDS and kernels["12x32_dense_z64"] == CC.REG
    assert kernels["12x32_dense_z256"] == CC.WIDE256 and kernels["2x3_z128"] == CC.WIDE128
    # and a row of degree 32 is decoded to a stop in the middle by the register kernel and by the wide one
    assert {kernels[n] for n in CC.ONE_DEGREE_32_ROW if n in sum(seen.values(), [])} == {CC.REG, CC.WIDE256}


def test_load_cases_reuse_the_decoded_codewords():
    for name in CC.LOAD_CASES:
        sh, Z, llr, (rb, ra, ri) = CC.load_case(name)
        assert len(llr) == len(ri) == CC.LOAD_CODEWORDS and (ri > 0).any() and (ri < 0).any()
        assert rb.shape == (5, (sh.shape[1] - sh.shape[0]) * Z) and ra.shape == llr.shape
    assert CC.N_LOAD % 2 == 1 and CC.N_LOAD > 2 * 256 * 6


@pytest.mark.parametrize("name", [n for n, c in CC.DECODER_CASES.items() if c[2] == 64])
def test_z64_restatements_agree_on_the_custom_codes(name):
    sh, _, llr = CC.decoder_case(name)
    b0, a0, i0 = R64.decode(sh, llr, CC.MAX_ITER)
    b1, a1, i1 = CC.decoder_ref(name)
    assert np.array_equal(i0, i1) and np.array_equal(b0, b1)
    assert np.array_equal(a0.view(np.int32), a1.view(np.int32))


# ---- special values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.SPECIAL_CASES))
def test_special_values_do_what_they_were_planted_for(name):
    sh, Z, llr = CC.special_case(name)
    k = {kind: i for i, kind in enumerate(CC.SPECIAL_KINDS)}
    assert llr.shape == (7, sh.shape[1] * Z) and sh.shape == CC.SPECIAL_CASES[name][:2]
    assert CC.kernel_of(sh.shape[0], Z) == {"4x8_z64": CC.REG, "4x8_z256": CC.WIDE256, "13x14_z64": CC.LDS}[name]
    rb, ra, ri = CC.special_ref(name)
    _, a1, _ = CC.special_ref(name, 1)
    # the inputs
    assert np.isposinf(llr[k["plus_inf"]]).sum() == 12 and not np.isneginf(llr[k["plus_inf"]]).any()
    assert np.isneginf(llr[k["minus_inf"]]).sum() == 12 and not np.isposinf(llr[k["minus_inf"]]).any()
    members = CC.row_members(sh, Z, sh.shape[0] // 2, 5)
    both = llr[k["both_inf"]]
    assert np.isposinf(both[members]).any() and np.isneginf(both[members]).any() and np.isinf(both).sum() == len(members)
    assert np.isnan(llr[k["nan"]]).sum() == 3
    big = llr[k["near_flt_max"]]
    assert np.isfinite(big).all() and (np.abs(big) == np.float32(3e38)).sum() >= 4
    sub = llr[k["subnormal"]]
    assert (sub != 0).all() and (np.abs(sub) < FLT_MIN_NORMAL).all()
    mz = llr[k["minus_zero"]]
    assert ((mz == 0) & np.signbit(mz)).sum() == 40
    # what the restatement makes of them
    assert np.isnan(a1[k["both_inf"]]).any()                                  # inf - inf in the first iteration already
    assert np.isnan(ra[k["both_inf"]]).any() and np.isnan(ra[k["nan"]]).any()
    assert not np.isfinite(a1[k["near_flt_max"]]).all()                       # finite input, overflow in q + R
    s1 = a1[k["subnormal"]]
    assert ((s1 != 0) & (np.abs(s1) < FLT_MIN_NORMAL)).sum() >= s1.size // 2  # APP after one iteration is subnormal:
    assert not np.array_equal(s1, sub)                                        # ... and not the input passed through
    for kind in ("plus_inf", "minus_inf", "subnormal", "minus_zero"):
        assert not np.isnan(ra[k[kind]]).any(), kind
    # +-0 decide 0: planting -0.0 is planting +0.0 as far as bits and iteration counts go
    plus = np.array(llr[k["minus_zero"]: k["minus_zero"] + 1])
    plus[plus == 0] = 0.0
    pb, _, pi = CC.quiet_decode(sh, plus, CC.SPECIAL_MAX_ITER, Z)
    assert pi[0] == ri[k["minus_zero"]] and np.array_equal(pb[0], rb[k["minus_zero"]])


# ---- encoder ----------------------------------------------------------------------------------------------------
def test_encoder_shapes_cover_what_the_case_list_says():
    seen = set()
    for Z in (64, 128, 256):
        assert CC.encoder_xs(Z) == (0, 1, Z // 2, Z - 1)
        for shape, (mb, nb, mid, row0_empty) in CC.ENCODER_SHAPES.items():
            for x in CC.encoder_xs(Z):
                sh = CC.encoder_table(shape, Z, x)
                assert sh.shape == (mb, nb) and RZ.dual_diagonal(sh) == (x, mid)
                seen.add((mb, nb - mb, mid, row0_empty))
    assert {(3, 1, 1, False), (3, 29, 1, False), (12, 12, 1, False), (12, 12, 10, False)} <= seen
    assert any(row0_empty for *_, row0_empty in seen)


@pytest.mark.parametrize("Z", [64, 128, 256])
def test_restated_encoder_satisfies_the_expanded_h(Z):
    """For the small codes (n <= 1024) H is formed and H c^T = 0 is checked on it; for every shape by circulant addressing."""
    small = 0
    for shape in CC.ENCODER_SHAPES:
        for x in CC.encoder_xs(Z):
            sh = CC.encoder_table(shape, Z, x)
            msg = CC.messages(sh, Z, 5, seed=x + 1)
            cw = RZ.encode(sh, msg, Z)
            assert np.array_equal(cw[:, : msg.shape[1]], msg) and not RZ.syndrome(sh, cw, Z).any()
            if cw.shape[1] <= 1024:
                small += 1
                H = RZ.expand(sh, Z).astype(np.int64)
                assert not ((H @ cw.T.astype(np.int64)) % 2).any()
    assert small == 4                                      # 3 x 4 at every x (n = 4 Z <= 1024)
    for name in ("3x5_z64", "4x8_wrap_dd_z256"):
        sh, z, _ = CC.decoder_case(name)
        if z != Z:
            continue
        cw = RZ.encode(sh, CC.messages(sh, Z, 5, seed=2), Z)
        assert not RZ.syndrome(sh, cw, Z).any()
        if cw.shape[1] <= 1024:
            assert not ((RZ.expand(sh, Z).astype(np.int64) @ cw.T.astype(np.int64)) % 2).any()


def test_message_bytes_above_bit_0_are_masked_by_the_restatement():
    sh = CC.encoder_table("3x4", 64, 1)
    raw = np.random.default_rng(6).choice(np.array([0, 1, 2, 3, 0xFE, 0xFF], dtype=np.uint8), size=(5, 64))
    assert np.array_equal(RZ.encode(sh, raw, 64), RZ.encode(sh, raw & 1, 64)) and RZ.encode(sh, raw, 64).max() == 1


# ---- outer code -------------------------------------------------------------------------------------------------
def test_outer_cases_reach_every_instantiation_and_block_size():
    T = CC
    rt = lambda R: next(t for t in (1, 2, 4, 8, 16) if R <= t)
    full = {rt(R) for _, R in T.OUTER_CODES if R == rt(R)} | {1, 4, 16}       # (R = 1, 4, 16: tests/test_outer_gpu.py)
    part = {rt(R) for _, R in T.OUTER_CODES if R < rt(R)} | {4}               # (R = 3 there)
    assert full == {1, 2, 4, 8, 16} and part == {4, 8, 16}                    # RT = 1, 2 have no R < RT
    for G, R in T.OUTER_CODES:
        O.check_geometry(G, R, 8)
    q = lambda nbytes: (nbytes + 3) // 4
    assert [q(b) for b in T.LONG_ROWS] == [255, 256, 256, 257, 513]
    assert [q(b) for b in T.STEP_ROWS] == [64, 65, 128, 129, 192]
    threads = lambda Q: 256 if Q >= 256 else (Q + 63) // 64 * 64               # the rule of gf3_outer_recover
    assert {threads(q(b)) for b in T.LONG_ROWS + T.STEP_ROWS} == {64, 128, 192, 256}
    assert -(-513 // 256) == 3 and 1021 % 4 and 1025 % 4                      # a third trip; partial lane items
