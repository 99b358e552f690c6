"""The per-codeword CRC-32 without a GPU: the restatement tests/crc_ref.py (self-consistency, the bit order anchored on
CRC-32's check value), the ABI names, the façade's refusal and the two report keys."""
import zlib

import numpy as np
import pytest

from tests import crc_ref as C


@pytest.mark.parametrize("k", [40, 768])
def test_restatement_attach_then_check_is_clean_and_every_single_flip_is_seen(k):
    rng = np.random.default_rng(k)
    payload = rng.integers(0, 2, size=(3, k - 32), dtype=np.uint8)
    msg = C.attach(payload, k)
    assert msg.shape == (3, k) and np.array_equal(msg[:, : k - 32], payload)
    got, bad, iters = C.check(msg, k, [1, 50, -50])
    assert np.array_equal(got, payload) and not bad.any() and iters.tolist() == [1, 50, -50]
    flipped = np.repeat(msg[:1], k, axis=0)                    # row i: bit i of row 0 flipped, payload and field alike
    flipped[np.arange(k), np.arange(k)] ^= 1
    got, bad, iters = C.check(flipped, k, np.full(k, 3))
    assert bad.all() and (iters == -3).all() and np.array_equal(got, flipped[:, : k - 32])
    assert C.check(flipped, k, np.full(k, -50))[2].tolist() == [-50] * k


def test_field_bit_order_is_anchored_on_the_check_value():
    """CRC-32("123456789") = 0xCBF43926.  The nine bytes, most significant bit first, are a payload of 72 bits (k = 104);
    the field is that value, bit 31 first."""
    assert zlib.crc32(b"123456789") == 0xCBF43926
    payload = np.unpackbits(np.frombuffer(b"123456789", dtype=np.uint8))
    msg = C.attach(payload[None], 104)[0]
    assert np.array_equal(msg[:72], payload)
    assert int("".join(map(str, msg[72:])), 2) == 0xCBF43926
    assert msg[72:].tolist() == [(0xCBF43926 >> (31 - i)) & 1 for i in range(32)]


def test_restatement_refuses_what_the_library_refuses():
    for k in (32, 36, 44, 7944):
        with pytest.raises(ValueError):
            C.check_k(k)
    for k in (40, 776, 7936):
        C.check_k(k)


def test_abi_names():
    from gf3_audio_modem_amd import _lib
    assert {"gf3_crc_attach", "gf3_crc_check"} <= set(_lib.exported_names())


def test_package_exports():
    import gf3_audio_modem_amd as pkg
    from gf3_audio_modem_amd import crc
    assert crc.CRC_BITS == 32 and pkg.CodewordCRC is crc.CodewordCRC


def test_codeword_crc_is_refused_on_other_encodings():
    from gf3_audio_modem_amd.coding import CodedChain
    from gf3_audio_modem_amd.OFDM import receiver
    make = lambda *a, **kw: None
    chain = CodedChain("XOR", 1536, 50, "csi", False, False, None, per_packet=2800, make_code=make, codeword_crc=True)
    with pytest.raises(ValueError, match="codeword_crc needs a 'QCLDPC-\\*' encoding"):
        chain.rate()
    assert CodedChain("XOR", 1536, 50, "csi", False, False, None, per_packet=2800, make_code=make).rate() is None
    assert CodedChain("QCLDPC-1/2", 1536, 50, "csi", False, False, None, 2800, make, True).rate() == "1/2"
    rx = receiver("A2", encoding="XOR")
    assert rx.codeword_crc is False
    rx.codeword_crc = True
    with pytest.raises(ValueError, match="codeword_crc"):
        rx.encode(np.zeros(100, dtype=int))
    with pytest.raises(ValueError, match="codeword_crc"):
        rx.decode(np.zeros(100, dtype=int))
    with pytest.raises(ValueError, match="codeword_crc"):
        rx.receive(np.zeros(100000))


def test_report_with_the_flags():
    from gf3_audio_modem_amd.coding import decode_report
    # 18 members of NG = 3 groups of (4, 2), then 3 rows of fill: the decoder's own counts and the CRC flags.  Rows 1 and
    # 16 converged on something wrong; rows 2, 7, 12 .. 14 and the fill did not converge (their CRC is bad as well, which
    # is not what the new keys count); row 19 is fill that happened to converge on something wrong.
    iters = np.array([1, 2, -50, 1, 1, 3, 1, -50, 1, 1, 1, 1, -50, -50, -50, 1, 50, 1, -50, 4, -50], dtype=np.int32)
    bad = np.array([0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 0, 1, 0, 1, 1, 1], dtype=np.uint8)
    plain = decode_report(iters, np.zeros(0, dtype=np.int32))
    assert list(plain) == ["codewords", "inner_failed", "recovered", "groups_failed", "failed_codewords"]
    rep = decode_report(iters, np.zeros(0, dtype=np.int32), None, bad)
    assert list(rep) == list(plain) + ["crc_failed", "crc_failed_codewords"]
    for key in plain:
        assert np.array_equal(rep[key], plain[key])
    assert rep["failed_codewords"].tolist() == [2, 7, 12, 13, 14, 18, 20] and rep["inner_failed"] == 7
    assert rep["crc_failed"] == 3 and type(rep["crc_failed"]) is int
    assert rep["crc_failed_codewords"].tolist() == [1, 16, 19] and rep["crc_failed_codewords"].dtype == np.int64
    status = np.array([2, 1, -3], dtype=np.int32)
    plain = decode_report(iters, status, (4, 2))
    rep = decode_report(iters, status, (4, 2), bad)
    assert set(plain) == {"codewords", "inner_failed", "recovered", "groups_failed", "failed_codewords"}
    assert set(rep) == set(plain) | {"crc_failed", "crc_failed_codewords"}
    for key in plain:
        assert np.array_equal(rep[key], plain[key])
    assert (rep["codewords"], rep["inner_failed"], rep["recovered"], rep["groups_failed"]) == (18, 5, 3, 1)
    assert rep["crc_failed"] == 2 and rep["crc_failed_codewords"].tolist() == [1, 16]     # truncated to the groups' members
    clean = decode_report(iters, status, (4, 2), np.zeros(21, dtype=np.uint8))
    assert clean["crc_failed"] == 0 and clean["crc_failed_codewords"].tolist() == []
