"""QC-LDPC coding on the GPU: the HIP encoder and layered min-sum decoder bit for bit against the NumPy restatement
(tests/ldpc_ref.py), the CSI-weighted soft demapper against NumPy, and the "QCLDPC-*" encodings end to end through
the façade."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import ldpc_ref as R
from tests.util import load, params_of

pytestmark = pytest.mark.gpu
RATES = ["1/2", "2/3", "3/4", "5/6"]


def code(rate=None, shifts=None):
    from gf3_audio_modem_amd import QCLDPC
    return QCLDPC(rate, shifts=shifts) if shifts is not None else QCLDPC(rate)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("n_cw", [1, 7, 4096])
def test_encoder_matches_restatement(rate, n_cw):
    q = code(rate)
    assert (q.n, q.k) == (1536, (24 - q.shifts.shape[0]) * 64)
    msg = np.random.default_rng(n_cw).integers(0, 2, size=(n_cw, q.k), dtype=np.uint8)
    cw = q.encode(torch.from_numpy(msg)).cpu().numpy()
    assert np.array_equal(cw, R.encode(q.shifts, msg))


def noisy_llrs(shifts, B, seed):
    """Codewords over BPSK/AWGN from clean to hopeless, with exact zeros and exact ties planted."""
    mb, nb = shifts.shape
    rng = np.random.default_rng(seed)
    cw = R.encode(shifts, rng.integers(0, 2, size=(B, (nb - mb) * 64), dtype=np.uint8))
    sig = np.linspace(0.3, 1.6, B)[:, None]
    llr = ((1.0 - 2.0 * cw + rng.normal(size=cw.shape) * sig) * 2.0 / sig ** 2).astype(np.float32)
    llr[:, rng.choice(cw.shape[1], 40, replace=False)] = 0.0
    t = rng.choice(cw.shape[1], 60, replace=False)
    llr[:, t[:30]] = 1.5
    llr[:, t[30:]] = -1.5
    llr[-1] = np.round(llr[-1])                          # many ties among the magnitudes
    return llr


def check_decoder(q, llr, max_iter):
    bits, app, its = q.decode(torch.from_numpy(llr), max_iter=max_iter, want_app=True, want_iters=True)
    rb, ra, ri = R.decode(q.shifts, llr, max_iter)
    assert np.array_equal(its.cpu().numpy(), ri)
    assert np.array_equal(bits.cpu().numpy(), rb)
    assert np.array_equal(app.cpu().numpy().view(np.int32), ra.view(np.int32))        # bit for bit
    return ri


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("max_iter", [1, 10, 50])
def test_decoder_matches_restatement_exactly(rate, max_iter):
    q = code(rate)
    ri = check_decoder(q, noisy_llrs(q.shifts, 48, seed=len(rate) + max_iter), max_iter)
    if max_iter == 50:
        assert (ri > 0).any() and (ri < 0).any()            # both stop rules were exercised


def test_decoder_without_optional_outputs_and_zero_llrs():
    q = code("1/2")
    llr = noisy_llrs(q.shifts, 9, seed=3)
    llr[0] = 0.0                                            # all-zero input: decisions 0, syndrome 0 after one pass
    bits = q.decode(torch.from_numpy(llr), max_iter=10).cpu().numpy()
    rb, _, ri = R.decode(q.shifts, llr, 10)
    assert np.array_equal(bits, rb) and ri[0] == 1 and not bits[0].any()


def test_decoder_many_block_rows_and_non_encodable_code():
    """A code of more than 12 block rows (check-message state in LDS) without the dual-diagonal parity part: it
    decodes exactly as the restatement, and encoding is refused."""
    rng = np.random.default_rng(21)
    mb, nb = 16, 24
    sh = np.where(rng.random((mb, nb)) < 0.3, rng.integers(0, 64, (mb, nb)), -1).astype(np.int16)
    for i in range(mb):
        sh[i, (i, i + 8)] = rng.integers(0, 64, 2)
    assert R.dual_diagonal(sh) is None
    q = code(shifts=sh)
    assert (q.n, q.k) == (1536, 512)
    llr = rng.normal(1.5, 2.0, size=(13, 1536)).astype(np.float32)
    for it in (1, 10):
        check_decoder(q, llr, it)
    with pytest.raises(ValueError, match="dual-diagonal"):
        q.encode(torch.zeros((1, q.k), dtype=torch.uint8))


def test_create_validation():
    from gf3_audio_modem_amd import _lib
    lib = _lib.load()
    sh = np.zeros((4, 24), dtype=np.int16)
    h = C.c_void_p()
    args = lambda t: t.ctypes.data_as(C.c_void_p)
    assert lib.gf3_ldpc_create(4, 24, 32, args(sh), C.byref(h)) == _lib.GF3_EINVAL
    assert b"Z=32" in lib.gf3_last_error(None)
    big = np.zeros((4, 33), dtype=np.int16)
    assert lib.gf3_ldpc_create(4, 33, 64, args(big), C.byref(h)) == _lib.GF3_EINVAL
    assert lib.gf3_ldpc_create(24, 24, 64, args(np.zeros((24, 24), np.int16)), C.byref(h)) == _lib.GF3_EINVAL
    bad = sh.copy()
    bad[1, 3] = 64
    assert lib.gf3_ldpc_create(4, 24, 64, args(bad), C.byref(h)) == _lib.GF3_EINVAL
    bad[1, 3] = -2
    assert lib.gf3_ldpc_create(4, 24, 64, args(bad), C.byref(h)) == _lib.GF3_EINVAL
    with pytest.raises(ValueError, match="max_iter"):
        code("1/2").decode(torch.zeros(1536), max_iter=0)


@pytest.mark.parametrize("name", ["g2_n4096_qpsk", "g3_n4096_16qam_gr5"])
def test_soft_demap_csi_matches_numpy(name):
    from gf3_audio_modem_amd import Engine, RxConfig
    g = load(name)
    p = params_of(g)
    eng = Engine(RxConfig(N=p.N, CP=p.CP, P=p.P, D=p.D, data_bins=p.data_carriers, const_points=p.const_points,
                          const_bits=p.const_bits, known_bits=p.known_bits, in_dtype=torch.float64,
                          fit_lo=p.fit_lo, fit_hi=p.fit_hi))
    x = torch.from_numpy(g["r"]).cuda()
    starts = (eng.sync_stream(x) + 2)[:-1]
    o = eng.demod_frames(x, starts, want=("eq", "Hs", "He", "Hest"))
    llr = eng.soft_demap_csi(o["eq"], o["Hs"], o["He"]).cpu().numpy()
    eq = o["eq"].cpu().numpy()
    Hest = o["Hest"].cpu().numpy()[:, :, np.asarray(p.data_carriers) - 1].reshape(eq.shape)
    ref = orc.soft_demap_maxlog(eq, 1.0, p) * (np.abs(Hest) ** 2)[..., None]
    assert llr.shape == (ref.size,)
    np.testing.assert_allclose(llr, ref.reshape(-1), rtol=1e-6, atol=1e-9 * np.abs(ref).max())
    assert np.array_equal(llr < 0, ref.reshape(-1) < 0)


# ---- end to end through the façade ------------------------------------------------------------------------------
def _roundtrip(channel, snr_db):
    from gf3_audio_modem_amd.OFDM import receiver
    rng = np.random.default_rng(2026)
    payload = rng.integers(0, 2, size=150_000)
    np.random.seed(17)                                     # the transmitter's fill draws
    tx = receiver("A2", encoding="QCLDPC-1/2")
    coded = np.asarray(tx.encode(payload))
    np.random.seed(17)
    sig = tx.transmit(payload)
    if channel is not None:
        from scipy.signal import lfilter
        sig = lfilter(channel, 1.0, sig)
    # silence before and after, as in a recording (a stream that ends with its last chirp has no detectable end:
    # the reference's peak rule drops every detection then); noise at snr_db below the signal's power
    sig = np.concatenate([np.zeros(2000), sig, np.zeros(2000)])
    noisy = sig + rng.normal(0, np.sqrt(np.mean(sig[2000:-2000] ** 2) / 10 ** (snr_db / 10)), sig.shape)
    raw, _, _ = receiver("A2", encoding="None").receive(noisy)
    raw_errors = int(np.sum(raw[: len(coded)] != coded))
    out, Hs0, He0 = receiver("A2", encoding="QCLDPC-1/2").receive(noisy)
    return payload, out, raw_errors, Hs0


def test_facade_qcldpc_corrects_awgn_errors():
    payload, out, raw_errors, Hs0 = _roundtrip(None, snr_db=7.0)
    assert raw_errors > 0                                  # the uncoded stream has bit errors at this SNR
    assert out.dtype == np.int64 and len(out) % 768 == 0 and len(out) >= len(payload)
    assert np.array_equal(out[: len(payload)], payload)
    assert not out[len(payload): -(-len(payload) // 768) * 768].any()     # the zero padding of the last codeword
    assert Hs0.shape == (2047,)


def test_facade_qcldpc_over_gr5_channel():
    """The measured 30-tap channel (gr5channel.csv, carried in the g3 fixture): the uncoded residual sits on the carriers
    in the channel's nulls, which the CSI weights mark as unreliable.  (At 30 dB; with this seed at 20 dB the
    equaliser's phase-slope fit itself fails -- half of the raw bits wrong, beyond any code.)"""
    payload, out, raw_errors, _ = _roundtrip(channel=load("g3_n4096_16qam_gr5")["channel"], snr_db=30.0)
    assert raw_errors > 0
    assert np.array_equal(out[: len(payload)], payload)


def test_facade_hard_decode_chain():
    """The reference's demap -> PS -> decode chain on a clean QC-LDPC stream (hard-input decoding)."""
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2", encoding="QCLDPC-3/4")
    payload = np.random.default_rng(8).integers(0, 2, size=10_000)
    coded = np.asarray(rx.encode(payload))
    flips = coded.copy()
    flips[::700] ^= 1                                      # a few hard errors
    out = rx.decode(rx.PS(flips))
    assert np.array_equal(out[: len(payload)], payload)


def test_facade_error_paths():
    from gf3_audio_modem_amd.OFDM import receiver
    np.random.seed(1)
    sig = receiver("A2", encoding="None").transmit(np.zeros(1000, dtype=np.int64))
    sig = np.concatenate([np.zeros(100), sig, np.zeros(100)])
    with pytest.raises(NotImplementedError, match="LDPC decoding is out of scope"):
        receiver("A2", encoding="LDPC").receive(sig)
    rx = receiver("A2", encoding="QCLDPC-1/2")
    rx.host_chunk_samples = 1 << 20
    with pytest.raises(NotImplementedError, match="piece-wise host path"):
        rx.receive(np.zeros(100_000))
