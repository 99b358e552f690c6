"""Longer QC-LDPC codes on the GPU (lifting sizes 128 and 256: Z/64 waves share a codeword): the HIP encoder and layered
min-sum decoder bit for bit against the Z-parameterised NumPy restatement (tests/ldpc_ref_z.py), the refusals of
gf3_ldpc_create, the Z = 64 path unchanged, and `ldpc_n` end to end through the façade."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import ldpc_ref as R64
from tests import ldpc_ref_z as RZ

pytestmark = pytest.mark.gpu
RATES = ["1/2", "2/3", "3/4", "5/6"]
# Eb/N0 (dB) at which the Z = 64 code of each rate is just past its waterfall (tests/test_ldpc_cpu.py); the longer codes
# decode there in a handful of iterations
WATERFALL_DB = {"1/2": 2.0, "2/3": 3.0, "3/4": 3.5, "5/6": 4.0}


def code(rate=None, shifts=None, Z=64):
    from gf3_audio_modem_amd import QCLDPC
    return QCLDPC(rate, shifts=shifts, Z=Z) if shifts is not None else QCLDPC(rate, Z=Z)


def five_llrs(sh, Z, ebn0_db, seed):
    """The five codewords of a launch: noiseless; two at moderate noise (Eb/N0 - 0.5 and + 0.75 dB); one at heavy noise
    (- 5 dB: never converges); one with exact zeros and exact ties (rounded to integers, values planted)."""
    mb, nb = sh.shape
    rate = (nb - mb) / nb
    rng = np.random.default_rng(seed)
    cw = RZ.encode(sh, rng.integers(0, 2, size=(5, (nb - mb) * Z), dtype=np.uint8), Z)
    sig = np.sqrt(1.0 / (2 * rate * 10 ** ((ebn0_db + np.array([0.0, -0.5, 0.75, -5.0, 0.5])) / 10)))[:, None]
    llr = ((1.0 - 2.0 * cw + rng.normal(size=cw.shape) * sig) * 2.0 / sig ** 2).astype(np.float32)
    llr[0] = (1.0 - 2.0 * cw[0]) * 4.0
    llr[4, rng.choice(cw.shape[1], 40, replace=False)] = 0.0
    t = rng.choice(cw.shape[1], 60, replace=False)
    llr[4, t[:30]] = 1.5
    llr[4, t[30:]] = -1.5
    llr[4] = np.round(llr[4])                              # many ties among the magnitudes (+-1.5 round to +-2)
    llr[4, t[:8]] = 1.5
    return llr


@functools.lru_cache(maxsize=None)
def family_case(rate, Z):
    """(shift table, LLRs [5, n]) of one code of the committed families; shared, read-only."""
    from gf3_audio_modem_amd.ldpc import shift_table
    sh = shift_table(rate, Z)
    llr = five_llrs(sh, Z, WATERFALL_DB[rate], seed=Z + len(rate) + int(rate[0]))
    llr.setflags(write=False)
    return sh, llr


@functools.lru_cache(maxsize=None)
def family_ref(rate, Z, max_iter):
    sh, llr = family_case(rate, Z)
    return RZ.decode(sh, llr, max_iter, Z)


def decode_and_compare(q, llr, max_iter, ref):
    rb, ra, ri = ref
    bits, app, its = q.decode(torch.from_numpy(np.array(llr)), max_iter=max_iter, want_app=True, want_iters=True)
    assert np.array_equal(its.cpu().numpy(), ri)
    assert np.array_equal(bits.cpu().numpy(), rb)
    assert np.array_equal(app.cpu().numpy().view(np.int32), ra.view(np.int32))        # bit for bit


@pytest.mark.parametrize("Z", [128, 256])
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("max_iter", [1, 10, 50])
def test_decoder_matches_restatement_exactly(rate, Z, max_iter):
    sh, llr = family_case(rate, Z)
    q = code(rate, Z=Z)
    assert (q.n, q.k) == (24 * Z, (24 - sh.shape[0]) * Z)
    rb, ra, ri = family_ref(rate, Z, max_iter)
    if max_iter == 50:                                      # the five codewords are what they are meant to be
        assert ri[0] == 1 and ri[1] > 1 and ri[2] > 1 and ri[1] != ri[2] and ri[3] == -50, ri
    decode_and_compare(q, llr, max_iter, (rb, ra, ri))
    for b in range(5):                                      # the same, one codeword per launch
        decode_and_compare(q, llr[b:b + 1], max_iter, (rb[b:b + 1], ra[b:b + 1], ri[b:b + 1]))


def tiny_z128():
    """mb = 3, nb = 5 at Z = 128, dual-diagonal (x = 65), the message shifts from {0, 63, 64, 65, 127}: every read
    crosses the wave boundary or wraps at 128."""
    return np.array([[63, 64, 65, 0, -1],
                     [65, 127, 0, 0, 0],
                     [0, 64, 65, -1, 0]], dtype=np.int16)


def test_tiny_custom_code_z128():
    sh = tiny_z128()
    assert RZ.dual_diagonal(sh) == (65, 1)
    q = code(shifts=sh, Z=128)
    assert (q.n, q.k) == (640, 256)
    rng = np.random.default_rng(5)
    msg = rng.integers(0, 2, size=(5, 256), dtype=np.uint8)
    cw = q.encode(torch.from_numpy(msg)).cpu().numpy()
    assert np.array_equal(cw, RZ.encode(sh, msg, 128))
    assert not RZ.syndrome(sh, cw, 128).any()
    llr = five_llrs(sh, 128, 4.0, seed=9)
    for it in (1, 10, 50):
        decode_and_compare(q, llr, it, RZ.decode(sh, llr, it, 128))


@pytest.mark.parametrize("Z", [128, 256])
@pytest.mark.parametrize("rate", RATES)
def test_encoder_matches_restatement(rate, Z):
    q = code(rate, Z=Z)
    msg = np.random.default_rng(Z + len(rate)).integers(0, 2, size=(5, q.k), dtype=np.uint8)
    cw = q.encode(torch.from_numpy(msg))
    assert np.array_equal(cw.cpu().numpy(), RZ.encode(q.shifts, msg, Z))
    assert not RZ.syndrome(q.shifts, cw.cpu().numpy(), Z).any()
    bits, its = q.decode(1.0 - 2.0 * cw.float(), max_iter=10, want_iters=True)      # noiseless round trip
    assert np.array_equal(bits.cpu().numpy(), msg) and its.cpu().tolist() == [1] * 5


def test_create_refusals():
    from gf3_audio_modem_amd import _lib
    lib = _lib.load()
    sh = np.zeros((4, 24), dtype=np.int16)
    h = C.c_void_p()
    args = lambda t: t.ctypes.data_as(C.c_void_p)
    for Z in (96, 512):
        assert lib.gf3_ldpc_create(4, 24, Z, args(sh), C.byref(h)) == _lib.GF3_EINVAL
        assert f"Z={Z}".encode() in lib.gf3_last_error(None)
    for Z in (128, 256):
        bad = sh.copy()
        bad[1, 3] = Z                                       # a shift equal to Z
        assert lib.gf3_ldpc_create(4, 24, Z, args(bad), C.byref(h)) == _lib.GF3_EINVAL
        bad[1, 3] = Z - 1
        assert lib.gf3_ldpc_create(4, 24, Z, args(bad), C.byref(h)) == _lib.GF3_OK
        assert (lib.gf3_ldpc_n(h), lib.gf3_ldpc_k(h)) == (24 * Z, 20 * Z)
        lib.gf3_ldpc_destroy(h)
    # more than 12 block rows decode at Z = 64 only (include/gf3rx.h)
    assert lib.gf3_ldpc_create(13, 24, 128, args(np.zeros((13, 24), np.int16)), C.byref(h)) == _lib.GF3_EINVAL
    assert b"mb" in lib.gf3_last_error(None)
    with pytest.raises(ValueError, match="Z=96"):
        code(shifts=sh, Z=96)


def test_z64_is_untouched():
    from gf3_audio_modem_amd.ldpc import shift_table
    sh = shift_table("2/3")
    llr = five_llrs(sh, 64, WATERFALL_DB["2/3"], seed=4)
    for max_iter in (1, 50):
        rb, ra, ri = R64.decode(sh, llr, max_iter)
        for q in (code("2/3"), code("2/3", Z=64)):
            assert (q.n, q.k) == (1536, 1024) and np.array_equal(q.shifts, sh)
            decode_and_compare(q, llr, max_iter, (rb, ra, ri))
    assert ri[0] == 1 and ri[3] == -50


# ---- end to end through the façade ------------------------------------------------------------------------------
@pytest.mark.parametrize("interleave", [False, True])
def test_facade_ldpc_n_6144_corrects_awgn_errors(interleave):
    """One mode-A2 packet (504 000 coded bits = 82 codewords of 6144) at 7 dB: the uncoded decisions of the same samples
    have errors, receive() returns the payload."""
    from gf3_audio_modem_amd.OFDM import receiver

    def rx(encoding):
        r = receiver("A2", encoding=encoding)
        r.ldpc_n = 6144
        return r

    rng = np.random.default_rng(2026)
    payload = rng.integers(0, 2, size=250_000)
    tx = rx("QCLDPC-1/2")
    tx.interleave = interleave
    np.random.seed(17)                                     # the transmitter's fill draws
    coded = np.asarray(tx.encode(payload))
    assert len(coded) == 504_000
    np.random.seed(17)
    sig = tx.transmit(payload)
    sig = np.concatenate([np.zeros(2000), sig, np.zeros(2000)])
    noisy = sig + rng.normal(0, np.sqrt(np.mean(sig[2000:-2000] ** 2) / 10 ** (7.0 / 10)), sig.shape)
    raw, _, _ = receiver("A2", encoding="None").receive(noisy)
    assert int(np.sum(raw[: len(coded)] != coded)) > 0     # the uncoded stream has bit errors at this SNR
    out, _, _ = tx.receive(noisy)
    assert out.dtype == np.int64 and len(out) == 82 * 3072
    assert np.array_equal(out[: len(payload)], payload)
    assert not out[len(payload): 82 * 3072].any()          # the zero padding of the last codeword


def test_facade_ldpc_n_values():
    from gf3_audio_modem_amd.OFDM import receiver, transmitter
    assert transmitter("A2", encoding="QCLDPC-1/2").ldpc_n == 1536
    payload = np.random.default_rng(1).integers(0, 2, size=5000)
    for n in (1536, 3072, 6144):
        tx = transmitter("A2", encoding="QCLDPC-3/4")
        tx.ldpc_n = n
        np.random.seed(2)
        coded = np.asarray(tx.encode(payload))
        k = n * 3 // 4
        n_cw = -(-len(payload) // k)
        rx = receiver("A2", encoding="QCLDPC-3/4")
        rx.ldpc_n = n
        out = rx.decode(rx.PS(coded))                       # hard-input decoding of the clean stream
        assert np.array_equal(out[: len(payload)], payload) and not out[len(payload): n_cw * k].any()
    tx.ldpc_n = 2048
    with pytest.raises(ValueError, match="ldpc_n"):
        tx.encode(payload)
    rx.ldpc_n = 2048
    with pytest.raises(ValueError, match="ldpc_n"):
        rx.decode(coded)
