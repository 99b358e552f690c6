"""The per-codeword CRC-32 on the GPU: gf3_crc_attach / gf3_crc_check (CodewordCRC) against tests/crc_ref.py -- byte for
byte, the arithmetic is exact -- through the real LDPC codes, and `codeword_crc` end to end through the façade: a codeword
that decodes to a WRONG codeword is seen, erased and repaired by the outer code, which without the CRC spreads its errors.

Façade geometry as in tests/test_coding_chain_gpu.py: mode A3, no_pilots = 4, packet_length = 12, "QCLDPC-1/2" -> 21 600
coded bits per packet, 28 codewords in two packets, NG = 4 groups of (4, 2); member t of group g is codeword 4 t + g."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import crc_ref as C

pytestmark = pytest.mark.gpu
KS = (40, 776, 768, 1280, 5120, 7936)       # smallest; no multiple of 64; rates 1/2 and 5/6 at Z = 64; largest family k; largest
N_PAYLOAD = 11_000
NOISE_DB = 15.0


def _np(t):
    return t.cpu().numpy()


def _rows(rng, n_cw, k):
    """Payload rows: zeros, ones, a single one in the first bit, a single one in the last bit, random fill for the rest."""
    p = rng.integers(0, 2, size=(n_cw, k - 32), dtype=np.uint8)
    special = np.zeros((4, k - 32), dtype=np.uint8)
    special[1] = 1
    special[2, 0] = 1
    special[3, -1] = 1
    p[: min(4, n_cw)] = special[: min(4, n_cw)]
    return p


@pytest.mark.parametrize("k", KS)
def test_attach_matches_the_restatement(k):
    from gf3_audio_modem_amd import CodewordCRC
    crc = CodewordCRC(k)
    assert crc.k == k and crc.k_payload == k - 32
    rng = np.random.default_rng(k)
    for n_cw in (5, 257):
        p = _rows(rng, n_cw, k)
        msg = crc.attach(p)
        assert msg.dtype == torch.uint8 and tuple(msg.shape) == (n_cw, k)
        assert np.array_equal(_np(msg), C.attach(p, k)), n_cw
    for row in _rows(rng, 5, k):                                # n_cw = 1: each kind of row alone
        assert np.array_equal(_np(crc.attach(row)), C.attach(row[None], k))
    assert crc.attach(p.reshape(-1)).shape == (257, k)          # flat input
    assert crc.attach(np.zeros((0, k - 32), dtype=np.uint8)).numel() == 0
    with pytest.raises(ValueError, match="whole rows"):
        crc.attach(np.zeros(k - 31, dtype=np.uint8))


def test_check_sees_every_single_bit_flip():
    """One launch of 768 rows at k = 768, row i a valid row with bit i flipped (payload and field positions alike)."""
    from gf3_audio_modem_amd import CodewordCRC
    k = 768
    crc = CodewordCRC(k)
    rng = np.random.default_rng(7)
    msg = C.attach(rng.integers(0, 2, size=(k, k - 32), dtype=np.uint8), k)
    msg[np.arange(k), np.arange(k)] ^= 1
    payload, bad, iters = crc.check(msg)
    assert iters is None and bad.dtype == torch.uint8 and payload.dtype == torch.uint8
    assert _np(bad).tolist() == [1] * k
    assert np.array_equal(_np(payload), msg[:, : k - 32])
    ref = C.check(msg, k)
    assert np.array_equal(_np(payload), ref[0]) and np.array_equal(_np(bad), ref[1])


@pytest.mark.parametrize("k", KS)
def test_check_matches_the_restatement_on_mixed_rows(k):
    """Valid rows and rows with one to three flipped bits in one launch, iteration counts from {1, 3, 50, -50} on both."""
    from gf3_audio_modem_amd import CodewordCRC
    crc = CodewordCRC(k)
    rng = np.random.default_rng(1000 + k)
    for n_cw in (1, 5, 257):
        msg = C.attach(_rows(rng, n_cw, k), k)
        hurt = np.flatnonzero(rng.integers(0, 2, size=n_cw))
        if n_cw == 1:
            hurt = np.array([0])
        for r in hurt:
            msg[r, rng.choice(k, size=int(rng.integers(1, 4)), replace=False)] ^= 1
        iters = np.resize(np.array([1, 3, 50, -50, -50, 50, 3, 1], dtype=np.int32), n_cw)
        want_p, want_bad, want_it = C.check(msg, k, iters)
        assert set(np.flatnonzero(want_bad)) == set(hurt)
        dev_it = torch.from_numpy(iters.copy()).cuda()
        payload, bad, it = crc.check(msg, dev_it)
        assert it.data_ptr() == dev_it.data_ptr()               # a contiguous int32 device tensor: in place
        assert np.array_equal(_np(payload), want_p) and np.array_equal(_np(bad), want_bad), n_cw
        assert np.array_equal(_np(it), want_it), n_cw
        host_it = iters.copy()
        assert np.array_equal(_np(crc.check(msg, host_it)[2]), want_it) and np.array_equal(host_it, iters)   # copied


def test_iteration_counts_map_as_the_contract_says():
    from gf3_audio_modem_amd import CodewordCRC
    k = 768
    crc = CodewordCRC(k)
    good = C.attach(np.random.default_rng(3).integers(0, 2, size=(4, k - 32), dtype=np.uint8), k)
    bad = good.copy()
    bad[:, 5] ^= 1
    assert _np(crc.check(bad, [1, 3, 50, -50])[2]).tolist() == [-1, -3, -50, -50]
    assert _np(crc.check(good, [1, 3, 50, -50])[2]).tolist() == [1, 3, 50, -50]
    with pytest.raises(ValueError, match="iteration counts"):
        crc.check(good, [1, 2, 3])


def test_every_combination_of_null_outputs_and_two_runs_agree():
    from gf3_audio_modem_amd import _lib
    lib = _lib.load()
    k, n_cw = 776, 9
    rng = np.random.default_rng(5)
    msg = C.attach(rng.integers(0, 2, size=(n_cw, k - 32), dtype=np.uint8), k)
    msg[[1, 4, 8], [0, 775, 400]] ^= 1
    iters = np.array([2, 2, -50, 7, 50, 1, 1, 1, 3], dtype=np.int32)
    want_p, want_bad, want_it = C.check(msg, k, iters)
    d_msg = torch.from_numpy(msg).cuda()
    st = _lib.stream(d_msg.device)
    seen = []
    for run in range(2):
        for use_p, use_it, use_bad in itertools.product((False, True), repeat=3):
            p = torch.full((n_cw, k - 32), 7, dtype=torch.uint8, device="cuda") if use_p else None
            it = torch.from_numpy(iters.copy()).cuda() if use_it else None
            bad = torch.full((n_cw,), 7, dtype=torch.uint8, device="cuda") if use_bad else None
            assert lib.gf3_crc_check(_lib.ptr(d_msg), n_cw, k, _lib.ptr(p), _lib.ptr(it), _lib.ptr(bad), st) == _lib.GF3_OK
            if use_p:
                assert np.array_equal(_np(p), want_p)
            if use_it:
                assert np.array_equal(_np(it), want_it)
            if use_bad:
                assert np.array_equal(_np(bad), want_bad)
        seen.append((_np(p).tobytes(), _np(it).tobytes(), _np(bad).tobytes()))
    assert seen[0] == seen[1]
    assert np.array_equal(_np(d_msg), msg)                      # the input is only read
    # n_cw = 0 is a no-op, pointers or none
    assert lib.gf3_crc_check(None, 0, k, None, None, None, st) == _lib.GF3_OK
    assert lib.gf3_crc_attach(None, 0, k, None, st) == _lib.GF3_OK
    assert lib.gf3_crc_check(_lib.ptr(d_msg), 0, k, _lib.ptr(p), _lib.ptr(it), _lib.ptr(bad), st) == _lib.GF3_OK
    assert np.array_equal(_np(p), want_p) and np.array_equal(_np(it), want_it)


@pytest.mark.parametrize("k,n_cw", [(40, 51 * 2048 + 7), (768, 2 * 2 * 2048 + 3), (7936, 2048 + 3)])
def test_more_passes_than_workgroups(k, n_cw):
    """A launch has at most 2048 workgroups, each taking every 2048th pass of 51 / 2 / 1 rows at these k: here the later
    passes exist (the second trip of the loop, the other scan buffer, the prefetch past the last pass), and two runs agree."""
    from gf3_audio_modem_amd import CodewordCRC
    crc = CodewordCRC(k)
    rng = np.random.default_rng(k + 1)
    p = rng.integers(0, 2, size=(n_cw, k - 32), dtype=np.uint8)
    want = C.attach(p, k)
    msg = crc.attach(p)
    assert np.array_equal(_np(msg), want)
    assert torch.equal(crc.attach(p), msg)
    hurt = rng.choice(n_cw, size=97, replace=False)
    hurt[:3] = [0, n_cw - 1, n_cw - 2]
    want[hurt, rng.integers(0, k, size=97)] ^= 1
    iters = rng.choice(np.array([1, 3, 50, -50], dtype=np.int32), size=n_cw)
    want_p, want_bad, want_it = C.check(want, k, iters)
    assert want_bad.sum() == len(set(hurt.tolist()))
    a, b = crc.check(want, iters), crc.check(want, iters)
    for got in (a, b):
        assert np.array_equal(_np(got[0]), want_p) and np.array_equal(_np(got[1]), want_bad)
        assert np.array_equal(_np(got[2]), want_it)


@pytest.mark.parametrize("k", [2048, 2056, 3072, 4096, 4104, 4608])
def test_every_instantiation_at_its_edges(k):
    """A thread holds 1, 2 or 4 lane items of 8 bits: k / 8 = 256 is the last row length with one, 257 the first with two
    (129 threads per row, the last item of the second trip missing), 512 the last with two, 513 the first with four; 384 and
    576 are the rate-1/2 and rate-3/4 messages at Z = 256."""
    from gf3_audio_modem_amd import CodewordCRC
    crc = CodewordCRC(k)
    rng = np.random.default_rng(k)
    p = _rows(rng, 9, k)
    want = C.attach(p, k)
    assert np.array_equal(_np(crc.attach(p)), want)
    want[[1, 4, 8, 6], [0, k - 33, k - 32, k - 1]] ^= 1         # first and last payload bit, first and last field bit
    iters = np.array([1, 3, 50, -50, 2, 2, 50, 1, 7], dtype=np.int32)
    want_p, want_bad, want_it = C.check(want, k, iters)
    assert want_bad.tolist() == [0, 1, 0, 0, 1, 0, 1, 0, 1] and want_it.tolist() == [1, -3, 50, -50, -2, 2, -50, 1, -7]
    payload, bad, it = crc.check(want, iters)
    assert np.array_equal(_np(payload), want_p) and np.array_equal(_np(bad), want_bad) and np.array_equal(_np(it), want_it)


def test_refusals():
    from gf3_audio_modem_amd import CodewordCRC, _lib
    lib = _lib.load()
    d = torch.zeros(65536, dtype=torch.uint8, device="cuda")    # (never touched: every call below is refused)
    p = _lib.ptr(d)
    for k in (32, 36, 44, 7944):
        with pytest.raises(ValueError, match="gf3_crc_attach"):
            CodewordCRC(k)
        assert lib.gf3_crc_attach(p, 1, k, p, None) == _lib.GF3_EINVAL
        assert f"k={k}".encode() in lib.gf3_last_error(None)
        assert lib.gf3_crc_check(p, 1, k, p, p, p, None) == _lib.GF3_EINVAL
        assert b"gf3_crc_check" in lib.gf3_last_error(None)
    assert lib.gf3_crc_attach(None, 1, 768, p, None) == _lib.GF3_EINVAL
    assert lib.gf3_crc_attach(p, -1, 768, p, None) == _lib.GF3_EINVAL
    assert lib.gf3_crc_check(None, 1, 768, p, None, None, None) == _lib.GF3_EINVAL
    off = _lib.ptr(d[4:])                                       # not 8-byte aligned
    assert lib.gf3_crc_attach(off, 1, 768, p, None) == _lib.GF3_EINVAL
    assert lib.gf3_crc_check(p, 1, 768, off, None, None, None) == _lib.GF3_EINVAL
    assert not _np(d).any()


@pytest.mark.parametrize("rate,Z", [("1/2", 64), ("2/3", 64), ("3/4", 64), ("5/6", 64), ("1/2", 256)])
def test_through_the_ldpc_codes(rate, Z):
    """attach -> QCLDPC.encode -> noiseless LLRs -> decode -> check: clean, and the payload is back."""
    from gf3_audio_modem_amd import QCLDPC, CodewordCRC
    code = QCLDPC(rate, Z=Z)
    crc = CodewordCRC(code.k)
    p = np.random.default_rng(Z + code.k).integers(0, 2, size=(5, code.k - 32), dtype=np.uint8)
    msg = crc.attach(p)
    assert np.array_equal(_np(msg), C.attach(p, code.k))
    llr = 4.0 * (1.0 - 2.0 * code.encode(msg).float())
    dec, iters = code.decode(llr, max_iter=10, want_iters=True)
    payload, bad, it = crc.check(dec, iters)
    assert not _np(bad).any() and _np(it).tolist() == [1] * 5
    assert np.array_equal(_np(payload), p)


# ---- through the façade ---------------------------------------------------------------------------------------------
def _receiver(crc, outer=(4, 2)):
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A3", encoding="QCLDPC-1/2", no_pilots=4, packet_length=12)
    rx.outer_code, rx.codeword_crc = outer, crc
    return rx


@functools.lru_cache(maxsize=None)
def _payload():
    return np.random.default_rng(2026).integers(0, 2, size=N_PAYLOAD)


@functools.lru_cache(maxsize=None)
def _wrong_codeword():
    """(768 random message bits, their codeword): a valid LDPC codeword that is not what was sent and whose CRC is bad."""
    from gf3_audio_modem_amd import QCLDPC
    msg = np.random.default_rng(99).integers(0, 2, size=768, dtype=np.uint8)
    assert C.check(msg[None], 768)[1][0] == 1
    return msg, _np(QCLDPC("1/2").encode(msg)).reshape(-1).astype(np.int64)


def _injured(crc, also_coin_flips):
    """encode() of the payload with codeword 5 (group 1, member 1) swapped for another valid codeword and, if asked,
    codeword 9 (group 1, member 2) overwritten with coin flips."""
    tx = _receiver(crc)
    np.random.seed(17)
    coded = np.array(tx.encode(_payload()))
    assert len(coded) == 2 * 21_600
    coded[5 * 1536: 6 * 1536] = _wrong_codeword()[1]
    if also_coin_flips:
        coded[9 * 1536: 10 * 1536] = np.random.default_rng(3).integers(0, 2, size=1536)
    return coded


def test_facade_detects_and_repairs_a_miscorrection():
    rx = _receiver(True)
    out = rx.decode(_injured(True, False))
    rep = rx.last_decode_report
    print({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in rep.items()})
    assert out.dtype == np.int64 and len(out) == 4 * 4 * 736
    assert np.array_equal(out[:N_PAYLOAD], _payload()) and not out[N_PAYLOAD:].any()
    assert rep["inner_failed"] == 0 and rep["crc_failed"] == 1 and rep["crc_failed_codewords"].tolist() == [5]
    assert rep["recovered"] == 1 and rep["groups_failed"] == 0 and rep["codewords"] == 24
    assert rep["failed_codewords"].tolist() == []


def test_facade_repairs_a_miscorrection_beside_a_failed_codeword():
    """The spreading case: group 1 loses member 2 to the decoder and member 1 to the CRC; both are rewritten."""
    rx = _receiver(True)
    out = rx.decode(_injured(True, True))
    rep = rx.last_decode_report
    print({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in rep.items()})
    assert rep["inner_failed"] == 1 and rep["failed_codewords"].tolist() == [9]
    assert rep["crc_failed"] == 1 and rep["crc_failed_codewords"].tolist() == [5]
    assert rep["recovered"] == 2 and rep["groups_failed"] == 0
    assert np.array_equal(out[:N_PAYLOAD], _payload())


def test_control_without_the_crc_the_miscorrection_spreads_unreported():
    """The same two injuries with codeword_crc off on both ends: the payload comes back wrong and no report key says so."""
    rx = _receiver(False)
    out = rx.decode(_injured(False, True))
    rep = rx.last_decode_report
    print({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in rep.items()})
    assert len(out) == 4 * 4 * 768
    assert not np.array_equal(out[:N_PAYLOAD], _payload())
    assert set(rep) == {"codewords", "inner_failed", "recovered", "groups_failed", "failed_codewords"}


def test_receive_end_to_end():
    payload = _payload()
    for crc, keys, per_cw in ((True, 7, 736), (False, 5, 768)):
        tx = _receiver(crc)
        np.random.seed(17)
        sig = np.concatenate([np.zeros(2000), tx.transmit(payload), np.zeros(2000)])
        rms = np.sqrt(np.mean(sig[2000:-2000] ** 2))
        noisy = sig + np.random.default_rng(5).normal(0, rms / 10 ** (NOISE_DB / 20), sig.shape)
        rx = _receiver(crc)
        bits, _, _ = rx.receive(noisy)
        rep = rx.last_decode_report
        assert rx.no_packets == 2 and len(bits) == 16 * per_cw and bits.dtype == np.int64
        assert np.array_equal(bits[:N_PAYLOAD], payload)
        assert len(rep) == keys and rep["groups_failed"] == 0
        if crc:
            assert rep["crc_failed"] == 0 and rep["crc_failed_codewords"].tolist() == []
            assert rep["crc_failed_codewords"].dtype == np.int64
        else:
            assert set(rep) == {"codewords", "inner_failed", "recovered", "groups_failed", "failed_codewords"}
