"""Every LDPC and outer-code kernel variant at the edges of what gf3_ldpc_create and rs_geometry accept, bit for bit
against the NumPy restatements (tests/ldpc_ref_z.py, tests/outer_ref.py).  The cases and their references come from
tests/coding_cases.py; tests/test_coding_shapes_cpu.py proves from the restatements alone that they take the paths they
are meant to take.  Every comparison is exact equality; the only class comparison is NaN against NaN in the
special-value cases.  DESIGN.md §12 has the table kernel instantiation -> case."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import coding_cases as CC
from tests import ldpc_ref_z as RZ
from tests import outer_ref as O
from tests.test_outer_gpu import ERASED, GOOD, patterns

pytestmark = pytest.mark.gpu


def code(sh, Z):
    from gf3_audio_modem_amd import QCLDPC
    return QCLDPC(shifts=np.array(sh), Z=Z)


def _np(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def decode_and_compare(q, llr, max_iter, ref):
    rb, ra, ri = ref
    bits, app, its = q.decode(torch.from_numpy(np.array(llr)), max_iter=max_iter, want_app=True, want_iters=True)
    assert np.array_equal(_np(its), ri), (_np(its), ri)
    assert np.array_equal(_np(bits), rb)
    assert same_bits(_np(app), ra)                          # bit for bit


# ---- decoder shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.DECODER_CASES))
def test_decoder_shape_matches_the_restatement(name):
    sh, Z, llr = CC.decoder_case(name)
    rb, ra, ri = CC.decoder_ref(name)
    q = code(sh, Z)
    assert (q.n, q.k) == (sh.shape[1] * Z, (sh.shape[1] - sh.shape[0]) * Z)
    decode_and_compare(q, llr, CC.MAX_ITER, (rb, ra, ri))
    decode_and_compare(q, llr[:1], CC.MAX_ITER, (rb[:1], ra[:1], ri[:1]))     # the first codeword alone
    if RZ.dual_diagonal(sh) is None:
        with pytest.raises(ValueError, match="dual-diagonal"):
            q.encode(torch.zeros((1, q.k), dtype=torch.uint8))


@pytest.mark.parametrize("name", ["3x5_z64", "13x14_z64"])
def test_partial_last_workgroup_z64(name):
    """Launches of 1, 3, 4, 5 and 9 codewords: the register kernel holds four codewords per workgroup (a partial last
    one at 1, 3, 5, 9), the LDS-state kernel one."""
    sh, Z, llr = CC.decoder_case(name)
    rb, ra, ri = CC.decoder_ref(name)
    q = code(sh, Z)
    assert len(llr) >= 9
    for m in (1, 3, 4, 5, 9):
        decode_and_compare(q, llr[:m], CC.MAX_ITER, (rb[:m], ra[:m], ri[:m]))
        t = len(llr) - m                                    # ... and the last m
        decode_and_compare(q, llr[t:], CC.MAX_ITER, (rb[t:], ra[t:], ri[t:]))


def test_create_boundaries():
    from gf3_audio_modem_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    args = lambda t: t.ctypes.data_as(C.c_void_p)
    for mb, nb, Z in ((12, 32, 256), (31, 32, 64), (1, 2, 64), (1, 2, 256)):
        sh = np.zeros((mb, nb), dtype=np.int16)
        assert lib.gf3_ldpc_create(mb, nb, Z, args(sh), C.byref(h)) == _lib.GF3_OK
        assert (lib.gf3_ldpc_n(h), lib.gf3_ldpc_k(h)) == (nb * Z, (nb - mb) * Z)
        lib.gf3_ldpc_destroy(h)
    for Z in (64, 128, 256):
        sh = np.zeros((4, 8), dtype=np.int16)
        sh[2, 1:] = -1                                      # block row 2 keeps a single non-zero block
        assert lib.gf3_ldpc_create(4, 8, Z, args(sh), C.byref(h)) == _lib.GF3_EINVAL
        assert b"fewer than 2" in lib.gf3_last_error(None)
        sh[2, 5] = Z - 1                                    # two are enough
        assert lib.gf3_ldpc_create(4, 8, Z, args(sh), C.byref(h)) == _lib.GF3_OK
        lib.gf3_ldpc_destroy(h)
    with pytest.raises(ValueError, match="fewer than 2"):
        code(np.array([[0, -1, -1], [0, 0, 0]], dtype=np.int16), 64)


# ---- decoder under load -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.LOAD_CASES)
def test_decoder_under_load(name):
    """4099 codewords in one launch, copies of five that the restatement has decoded: workgroups queue and share compute
    units, and every copy must equal the reference row of its original."""
    sh, Z, llr, (rb, ra, ri) = CC.load_case(name)
    q = code(sh, Z)
    idx = torch.arange(CC.N_LOAD, device="cuda") % len(llr)
    x = torch.from_numpy(np.array(llr)).cuda()[idx]
    bits, app, its = q.decode(x, max_iter=CC.MAX_ITER, want_app=True, want_iters=True)
    i = _np(idx)
    assert np.array_equal(_np(its), ri[i])
    assert np.array_equal(_np(bits), rb[i])
    assert same_bits(_np(app), ra[i])


# ---- special values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.SPECIAL_CASES))
def test_special_values(name):
    """+-inf, both in one check row, NaN, values near FLT_MAX, subnormals and -0.0: iteration counts and decisions equal,
    APP bit for bit wherever the restatement is not NaN and NaN wherever it is (NaN payloads and signs are not compared:
    nothing downstream reads them)."""
    sh, Z, llr = CC.special_case(name)
    rb, ra, ri = CC.special_ref(name)
    q = code(sh, Z)
    for rows in (slice(None),) + tuple(slice(b, b + 1) for b in range(len(llr))):
        bits, app, its = q.decode(torch.from_numpy(np.array(llr[rows])), max_iter=CC.SPECIAL_MAX_ITER, want_app=True,
                                  want_iters=True)
        app, want = _np(app), ra[rows]
        kinds = CC.SPECIAL_KINDS[rows]
        assert np.array_equal(_np(its), ri[rows]), (kinds, _np(its), ri[rows])
        assert np.array_equal(_np(bits), rb[rows]), kinds
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(app), nan), kinds
        assert same_bits(np.where(nan, np.float32(0), app), np.where(nan, np.float32(0), want)), kinds


# ---- encoder shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z", [64, 128, 256])
@pytest.mark.parametrize("shape", list(CC.ENCODER_SHAPES))
def test_encoder_shape_matches_the_restatement(shape, Z):
    for x in CC.encoder_xs(Z):
        sh = CC.encoder_table(shape, Z, x)
        q = code(sh, Z)
        msg = CC.messages(sh, Z, 5, seed=x + 1)
        ref = RZ.encode(sh, msg, Z)
        for m in (1, 5):
            cw = q.encode(torch.from_numpy(msg[:m]))
            assert np.array_equal(_np(cw), ref[:m]), (x, m)
        assert not RZ.syndrome(sh, _np(cw), Z).any()
        bits, its = q.decode(1.0 - 2.0 * cw.float(), max_iter=10, want_iters=True)     # noiseless round trip
        assert np.array_equal(_np(bits), msg) and _np(its).tolist() == [1] * 5, x


@pytest.mark.parametrize("Z", [64, 128, 256])
def test_encoder_under_load(Z):
    sh = CC.encoder_table("12x24_mid10", Z, Z // 2)
    q = code(sh, Z)
    msg = CC.messages(sh, Z, 5, seed=Z)
    ref = RZ.encode(sh, msg, Z)
    idx = torch.arange(CC.N_LOAD, device="cuda") % 5
    cw = q.encode(torch.from_numpy(msg).cuda()[idx])
    assert np.array_equal(_np(cw), ref[_np(idx)])


@pytest.mark.parametrize("Z", [64, 128, 256])
def test_encoder_masks_message_bytes_to_bit_0(Z):
    sh = CC.encoder_table("3x32", Z, 1)
    q = code(sh, Z)
    raw = np.random.default_rng(Z).choice(np.array([0, 1, 2, 3, 0xFE, 0xFF], dtype=np.uint8), size=(5, q.k))
    cw = _np(q.encode(torch.from_numpy(raw)))
    assert np.array_equal(cw, RZ.encode(sh, raw & 1, Z))
    assert cw.max() == 1 and np.array_equal(cw[:, : q.k], raw & 1)           # the systematic part holds 0 / 1 only


# ---- outer code -------------------------------------------------------------------------------------------------
def recover_and_compare(G, R, nbytes, pats, seed):
    """One launch with one erasure pattern per group against the restatement: statuses, bits, the data restored in a
    repairable group whatever the erased rows held, every other row untouched.  Returns the statuses."""
    from gf3_audio_modem_amd import OuterRS
    k, NG = 8 * nbytes, len(pats)
    rs = OuterRS(G, R, k)
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2, size=(NG * G, k), dtype=np.uint8)
    par = O.encode(data, G, R)
    tx = np.concatenate([data.reshape(NG, G, k).transpose(1, 0, 2), par.reshape(NG, R, k).transpose(1, 0, 2)]).reshape(-1, k)
    iters = np.full(len(tx), GOOD, dtype=np.int32)
    rows = [t * NG + g for g, members in enumerate(pats) for t in members]
    iters[rows] = ERASED
    rx = tx.copy()
    rx[rows] = rng.integers(0, 2, size=(len(rows), k), dtype=np.uint8)       # the erased rows hold garbage
    ref, ref_status = O.recover(rx, iters, G, R)
    got, status = rs.recover(torch.from_numpy(rx).cuda(), iters)
    got = _np(got)
    assert np.array_equal(_np(status), ref_status), (_np(status), ref_status)
    assert np.array_equal(got, ref)
    for g, members in enumerate(pats):
        grp = np.arange(G + R) * NG + g
        e_d, e_p = sum(t < G for t in members), sum(t >= G for t in members)
        assert ref_status[g] == (0 if e_d == 0 else e_d if e_d <= R - e_p else -e_d)
        if ref_status[g] > 0:
            assert np.array_equal(got[grp[:G]], tx[grp[:G]])                  # the data is back
            assert np.array_equal(got[grp[G:]], rx[grp[G:]])                  # parity rows are never rewritten
        else:
            assert np.array_equal(got[grp], rx[grp])                          # byte-identical to the input
    return ref_status


@pytest.mark.parametrize("G,R", CC.OUTER_CODES)
def test_outer_encode_every_instantiation(G, R):
    """33 and 97 bytes per row: a partial lane item at the end of a row; NG in {1, 3}."""
    from gf3_audio_modem_amd import OuterRS
    rng = np.random.default_rng(G * 31 + R)
    for nbytes in (33, 97):
        rs = OuterRS(G, R, 8 * nbytes)
        for NG in (1, 3):
            msg = rng.integers(0, 2, size=(NG * G, 8 * nbytes), dtype=np.uint8)
            par = rs.encode(msg)
            assert tuple(par.shape) == (NG * R, 8 * nbytes)
            assert np.array_equal(_np(par), O.encode(msg, G, R)), (nbytes, NG)


@pytest.mark.parametrize("G,R", CC.OUTER_CODES)
def test_outer_recover_every_instantiation(G, R):
    rng = np.random.default_rng(G + 7 * R)
    pats = patterns(G, R)
    for _ in range(4):                                                        # random patterns, repairable or not
        pats.append(rng.choice(G + R, size=min(G + R, int(rng.integers(1, R + 3))), replace=False).tolist())
    if (G, R) in CC.EVERY_ED_CODES:
        for e_d in range(1, R + 1):                                           # every e_d: coefficient words that end mid-word
            pats.append(sorted(rng.choice(G, size=e_d, replace=False).tolist()))
            pats.append(sorted(rng.choice(G, size=e_d, replace=False).tolist()) + [G])      # ... with parity row 0 gone
    st = recover_and_compare(G, R, 33, pats, seed=G * R)
    e_d = [sum(t < G for t in members) for members in pats]
    assert st[0] == 0 and st[4] == 0 and st[1] == e_d[1] > 0 and st[2] == e_d[2] and st[3] == 1
    assert st[5] == -e_d[5] < 0 and st[6] == -G
    if (G, R) in CC.EVERY_ED_CODES:
        assert set(range(1, R + 1)) <= set(st.tolist())


@pytest.mark.parametrize("G,R", CC.ROW_CODES)
@pytest.mark.parametrize("nbytes", CC.LONG_ROWS + CC.STEP_ROWS)
def test_outer_row_lengths(G, R, nbytes):
    """Q = ceil(nbytes / 4) lane items per row: every step of the block-size rule of gf3_outer_recover (64, 128, 192, 256
    threads), the second and third trips of its streaming loop, and a partial lane item on the last trip."""
    from gf3_audio_modem_amd import OuterRS
    k = 8 * nbytes
    rs = OuterRS(G, R, k)
    rng = np.random.default_rng(nbytes + G)
    for NG in (1, 3):
        msg = rng.integers(0, 2, size=(NG * G, k), dtype=np.uint8)
        assert np.array_equal(_np(rs.encode(msg)), O.encode(msg, G, R)), NG
    full = list(range(R))                                                     # R data members
    mixed = [G - 1, G // 2] + [G + r for r in range(R - 2)]                   # e_d = 2, the last two parity rows chosen
    beyond = list(range(R)) + [G + R - 1]
    st = recover_and_compare(G, R, nbytes, [full], seed=nbytes)
    assert st.tolist() == [R]
    st = recover_and_compare(G, R, nbytes, [mixed, full, beyond], seed=nbytes + 1)
    assert st.tolist() == [2, R, -R]
