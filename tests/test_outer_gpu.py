"""The outer Reed-Solomon erasure code on the GPU: gf3_outer_encode / gf3_outer_recover (OuterRS) against the NumPy
restatement (tests/outer_ref.py) -- bit-exact, the arithmetic is exact -- and `outer_code` end to end through the façade
on the impulse scenario of tests/test_impulse_gpu.py."""
import numpy as np
import pytest
import torch

from tests import outer_ref as O

pytestmark = pytest.mark.gpu
ERASED, GOOD = -50, 3


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("G,R", [(1, 1), (2, 1), (5, 3), (20, 4), (239, 16)])
def test_encode_matches_the_restatement(G, R):
    """k / 8 in {1, 3, 96, 97, 640}: a lane owns four byte positions, so 1, 3 and 97 end in a partial lane item; 640 is more
    than one wave of lane items per row.  NG in {1, 3, 13}."""
    from gf3_audio_modem_amd import OuterRS
    rng = np.random.default_rng(G * 17 + R)
    for nbytes in (1, 3, 96, 97, 640):
        k = 8 * nbytes
        rs = OuterRS(G, R, k)
        for NG in (1, 3, 13):
            msg = rng.integers(0, 2, size=(NG * G, k), dtype=np.uint8)
            par = rs.encode(msg)
            assert par.dtype == torch.uint8 and tuple(par.shape) == (NG * R, k)
            assert np.array_equal(_np(par), O.encode(msg, G, R)), (nbytes, NG)
    assert rs.encode(np.zeros((0, k), dtype=np.uint8)).numel() == 0


def patterns(G, R):
    """Erased members per group, one pattern per group of one launch (clamped where G < R)."""
    d = lambda cnt: list(range(min(cnt, G)))                                  # the first cnt data members
    e_p = R // 2
    return [
        [],                                                                   # no erasure
        d(R) + [G + r for r in range(R - len(d(R)))],                         # R erasures, as many of them data as there are
        [G - 1 - j for j in range(min(R - e_p, G))] + [G + R - 1 - r for r in range(e_p)],     # mixed, e_d + e_p = R
        [G // 2] + [G + r for r in range(R - 1)],                             # the first parity rows erased: later rows are chosen
        [G + r for r in range(R)],                                            # only parity
        (d(R) + [G + R - 1]) if G >= R else (d(1) + [G + r for r in range(R)]),               # e_d = R - e_p + 1
        list(range(G + R)),                                                   # every member
    ]


@pytest.mark.parametrize("G,R,nbytes", [(1, 1, 3), (2, 1, 97), (5, 3, 1), (5, 3, 97), (20, 4, 96), (239, 16, 97), (20, 4, 640)])
def test_recover_matches_the_restatement(G, R, nbytes):
    from gf3_audio_modem_amd import OuterRS
    k = 8 * nbytes
    rs = OuterRS(G, R, k)
    rng = np.random.default_rng(G + R + nbytes)
    pats = patterns(G, R)
    for _ in range(4):                                                        # and some random patterns, repairable or not
        pats.append(rng.choice(G + R, size=min(G + R, int(rng.integers(1, R + 3))), replace=False).tolist())
    NG = len(pats)
    data = rng.integers(0, 2, size=(NG * G, k), dtype=np.uint8)
    par = O.encode(data, G, R)
    tx = np.concatenate([data.reshape(NG, G, k).transpose(1, 0, 2), par.reshape(NG, R, k).transpose(1, 0, 2)]).reshape(-1, k)
    iters = np.full(len(tx), GOOD, dtype=np.int32)
    rows = [t * NG + g for g, members in enumerate(pats) for t in members]
    iters[rows] = ERASED
    outs = []
    for garbage_seed in (1, 2):                                               # the erased rows hold garbage, twice another
        rx = tx.copy()
        rx[rows] = np.random.default_rng(garbage_seed).integers(0, 2, size=(len(rows), k), dtype=np.uint8)
        ref, ref_status = O.recover(rx, iters, G, R)
        dev = torch.from_numpy(rx).cuda()
        got, status = rs.recover(dev, iters)
        assert got.data_ptr() == dev.data_ptr() and status.dtype == torch.int32           # in place
        assert np.array_equal(_np(status), ref_status), (_np(status), ref_status)
        assert np.array_equal(_np(got), ref)
        outs.append((_np(got), rx))
    st = ref_status
    e_d = [sum(t < G for t in members) for members in pats]
    assert st[0] == 0 and st[4] == 0 and st[1] == e_d[1] > 0 and st[2] == e_d[2] and st[3] == 1
    assert st[5] == -e_d[5] < 0 and st[6] == -G
    for g in range(NG):
        grp = np.arange(G + R) * NG + g
        for got, rx in outs:
            if st[g] > 0:
                assert np.array_equal(got[grp[:G]], tx[grp[:G]])              # the data is back, whatever the garbage was
                assert np.array_equal(got[grp[G:]], rx[grp[G:]])              # parity rows are never rewritten
            else:
                assert np.array_equal(got[grp], rx[grp])                      # byte-identical to the input


def test_round_trip_through_the_inner_code():
    """OuterRS -> QCLDPC.encode -> noiseless LLRs with chosen codewords replaced -> decode(want_iters) -> recover.
    All-zero LLRs do not make this decoder fail (every decision is 0 and the all-zero word is a codeword: iters = 1), so
    the chosen codewords get random signs at full confidence instead; that they then report iters < 0 is asserted."""
    from gf3_audio_modem_amd import QCLDPC, OuterRS
    G, R, NG = 20, 4, 3
    code = QCLDPC("1/2")
    rs = OuterRS(G, R, code.k)
    rng = np.random.default_rng(11)
    msg = rng.integers(0, 2, size=(NG * G, code.k), dtype=np.uint8)
    data = torch.from_numpy(msg).cuda().reshape(NG, G, code.k)
    par = rs.encode(data).reshape(NG, R, code.k)
    sent = torch.cat([data.transpose(0, 1), par.transpose(0, 1)]).contiguous().reshape(-1, code.k)
    llr = 4.0 * (1.0 - 2.0 * code.encode(sent).float())
    lost = [0 * NG + 0, 5 * NG + 0, 19 * NG + 0, 21 * NG + 0,                 # group 0: three data members and a parity member
            7 * NG + 1,                                                       # group 1: one data member
            1 * NG + 2, 2 * NG + 2, 3 * NG + 2, 4 * NG + 2, 5 * NG + 2]       # group 2: five data members, beyond repair
    llr[lost] = torch.from_numpy(4.0 * (1.0 - 2.0 * rng.integers(0, 2, size=(len(lost), code.n)))).float().cuda()
    bits, iters = code.decode(llr, max_iter=10, want_iters=True)
    it = _np(iters)
    assert (it[lost] < 0).all() and (np.delete(it, lost) > 0).all()
    before = _np(bits).copy()
    fixed, status = rs.recover(bits, iters)
    assert _np(status).tolist() == [3, 1, -5]
    out = _np(fixed)[: NG * G].reshape(G, NG, code.k).transpose(1, 0, 2)
    want = msg.reshape(NG, G, code.k)
    assert np.array_equal(out[:2], want[:2])
    assert np.array_equal(_np(fixed).reshape(G + R, NG, code.k)[:, 2], before.reshape(G + R, NG, code.k)[:, 2])
    ref, ref_status = O.recover(before, it, G, R)
    assert np.array_equal(_np(fixed), ref) and np.array_equal(_np(status), ref_status)


def test_refusals():
    from gf3_audio_modem_amd import OuterRS, _lib
    from gf3_audio_modem_amd.OFDM import receiver
    lib = _lib.load()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")                   # (never touched: every call below is refused)
    p = _lib.ptr(d)
    for G, R, k in ((5, 0, 8), (5, 17, 8), (240, 16, 8), (5, 3, 12)):
        with pytest.raises(ValueError, match="gf3_outer_encode"):
            OuterRS(G, R, k)
        assert lib.gf3_outer_encode(p, 1, G, R, k, p, None) == _lib.GF3_EINVAL
        assert lib.gf3_outer_recover(p, p, 1, G, R, k, p, None) == _lib.GF3_EINVAL
        assert b"gf3_outer_recover" in lib.gf3_last_error(None)
    assert lib.gf3_outer_encode(None, 1, 5, 3, 8, p, None) == _lib.GF3_EINVAL
    assert lib.gf3_outer_encode(p, -1, 5, 3, 8, p, None) == _lib.GF3_EINVAL
    rs = OuterRS(5, 3, 16)
    with pytest.raises(ValueError, match="whole groups"):
        rs.encode(np.zeros((4, 16), dtype=np.uint8))
    with pytest.raises(ValueError, match="iteration counts"):
        rs.recover(np.zeros((8, 16), dtype=np.uint8), np.zeros(7, dtype=np.int32))
    bad = receiver("A2", encoding="XOR")
    bad.outer_code = (20, 4)
    with pytest.raises(ValueError, match="outer_code"):
        bad.encode(np.zeros(100, dtype=int))
    with pytest.raises(ValueError, match="outer_code"):
        bad.receive(np.zeros(100000))


# ---- end to end through the façade ------------------------------------------------------------------------------
def _stream(payload, outer, interleave=False):
    from gf3_audio_modem_amd.OFDM import receiver
    np.random.seed(17)
    tx = receiver("A2", encoding="QCLDPC-1/2")
    tx.outer_code = outer
    tx.interleave = interleave
    sig = tx.transmit(payload)
    return tx, np.concatenate([np.zeros(2000), sig, np.zeros(2000)])


def test_facade_outer_code_repairs_the_clicked_codewords():
    """Mode A2, "QCLDPC-1/2", 150 000 payload bits in one packet, white noise 15 dB below the signal, data symbols 70-72
    overwritten with white noise of 8 x the signal's rms, stream order, "csi" weights: codewords 127 .. 133 are hit
    (tests/test_outer_cpu.py restates the arithmetic), seven consecutive ones, one member each of seven of the 13 groups."""
    from gf3_audio_modem_amd.OFDM import receiver
    from tests.test_impulse_gpu import clicked
    payload = np.random.default_rng(2026).integers(0, 2, size=150_000)
    reports = {}
    for outer in (None, (20, 4)):
        tx, sig = _stream(payload, outer)
        noisy = clicked(sig, tx, 2000 + tx.chirp_length, 1.0)
        rx = receiver("A2", encoding="QCLDPC-1/2")
        assert rx.outer_code is None and rx.last_decode_report is None and rx.llr_weighting == "csi" and not rx.interleave
        rx.outer_code = outer
        out, Hs0, _ = rx.receive(noisy)
        rep = reports[outer] = rx.last_decode_report
        print(outer, {k: v for k, v in rep.items()})
        assert out.dtype == np.int64 and Hs0.shape == (2047,)
        assert rep["inner_failed"] == len(rep["failed_codewords"])
        if outer is None:                                   # (the 132 codewords of coin-flip fill count as failed here)
            assert len(out) == 328 * 768 and rep["codewords"] == 328
            hit = [c for c in rep["failed_codewords"].tolist() if c < 196]
            assert rep["inner_failed"] >= 1 and not np.array_equal(out[: len(payload)], payload)
            assert len(hit) >= 1 and set(hit) <= set(range(127, 134))
            assert rep["recovered"] == 0 and rep["groups_failed"] == 0
        else:
            assert rep["codewords"] == 312 and set(rep["failed_codewords"].tolist()) <= set(range(127, 134))
            assert len(out) == 13 * 20 * 768
            assert np.array_equal(out[: len(payload)], payload) and not out[len(payload):].any()
            assert rep["groups_failed"] == 0 and rep["recovered"] == rep["inner_failed"] >= 1


def test_facade_outer_code_with_interleaver_on_a_clean_packet_and_hard_decode():
    from gf3_audio_modem_amd.OFDM import receiver
    payload = np.random.default_rng(7).integers(0, 2, size=150_000)
    tx, sig = _stream(payload, (20, 4), interleave=True)
    rms = np.sqrt(np.mean(sig[2000:-2000] ** 2))
    noisy = sig + np.random.default_rng(5).normal(0, rms / 10 ** (15.0 / 20), sig.shape)
    rx = receiver("A2", encoding="QCLDPC-1/2")
    rx.outer_code, rx.interleave, rx.llr_weighting = (20, 4), True, "noise2d"
    out, _, _ = rx.receive(noisy)
    rep = rx.last_decode_report
    assert np.array_equal(out[: len(payload)], payload) and len(out) == 199_680
    assert rep["inner_failed"] == 0 and rep["recovered"] == 0 and rep["groups_failed"] == 0 and rep["codewords"] == 312
    assert rx.last_symbol_snr_db.shape == (1, 180)                            # (the other reports of the small copy are intact)
    # decode(), the hard-input path, on the coded bits themselves with codewords 40 .. 52 (13 = NG consecutive) replaced
    np.random.seed(17)
    coded = np.asarray(tx.encode(payload))
    plain = rx._engine().interleave(torch.from_numpy(coded.astype(np.uint8)), inverse=True).cpu().numpy()
    plain[40 * 1536: 53 * 1536] = np.random.default_rng(3).integers(0, 2, size=13 * 1536)
    hurt = rx._engine().interleave(torch.from_numpy(plain), inverse=False).cpu().numpy()
    dec = rx.decode(hurt)
    rep = rx.last_decode_report
    assert rep["failed_codewords"].tolist() == list(range(40, 53)) and rep["recovered"] == 13 and rep["groups_failed"] == 0
    assert np.array_equal(dec[: len(payload)], payload) and len(dec) == 199_680


def test_without_outer_code_receive_returns_what_it_returned():
    """outer_code = None: the bits are those of the direct engine calls followed by the decoder, which is what receive()
    was before the attribute existed (the form of tests/test_impulse_gpu.py's defaults test); the report is filled."""
    from gf3_audio_modem_amd import QCLDPC
    from gf3_audio_modem_amd.OFDM import receiver
    bits = np.random.default_rng(3).integers(0, 2, size=100_000)
    np.random.seed(5)
    tx = receiver("A2", encoding="QCLDPC-3/4")
    sig = np.concatenate([np.zeros(2000), tx.transmit(bits), np.zeros(2000)])
    noisy = sig + np.random.default_rng(4).normal(0, np.sqrt(np.mean(sig ** 2) / 10 ** 0.9), sig.shape)
    rx = receiver("A2", encoding="QCLDPC-3/4")
    eng = rx._engine(noisy.dtype)
    x = eng._samples(noisy)
    o = eng.demod_frames(x, (eng.sync_stream(x) + 2)[:-1], want=("eq", "Hs", "He"))
    llr = eng.soft_demap_csi(o["eq"], o["Hs"], o["He"])
    code = QCLDPC("3/4")
    want, its = code.decode(llr[: llr.numel() // code.n * code.n], max_iter=rx.ldpc_max_iter, want_iters=True)
    got, _, _ = rx.receive(noisy)
    assert np.array_equal(got, want.reshape(-1).cpu().numpy().astype(np.int64))
    rep = rx.last_decode_report
    assert rep["codewords"] == 328 and rep["failed_codewords"].tolist() == np.flatnonzero(_np(its) < 0).tolist()
    assert rep["recovered"] == 0 and rep["groups_failed"] == 0
