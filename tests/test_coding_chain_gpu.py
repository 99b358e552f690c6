"""receive() and decode() on the "QCLDPC-*" encodings against the coded chain written out by hand from the calls the
package exposes: sync_stream, demod_frames / demod_frames_llr, the demapper of the weighting, interleave(inverse=True),
QCLDPC.decode, OuterRS.recover on rows regrouped with transmitted_index in NumPy.  Every stage is deterministic, so the
comparison is np.array_equal throughout: returned bits, Hs / He of packet 0, the slopes, every key of
`last_decode_report`, `last_snr_db` and `last_symbol_snr_db` where the weighting defines them.

Geometry: mode A3 (900 carriers), no_pilots = 4, packet_length = 12 -> 21 600 coded bits per packet = 14 whole codewords
of 1536 and a rest, so a packet does not end on a codeword.  12 000 payload bits span two packets without an outer code
(16 codewords) and with (4, 2) (NG = 4 groups in the 28 codewords of two packets).  2000 zeros either side.

Noise: white, NOISE_DB = 15 dB below the signal.  At that level, in every configuration, the payload comes back AND
some codewords of the message take two decoder iterations (asserted: else the decoder and the outer code would be
compared on inputs that exercise neither).  The file uses only calls that predate coding.py and passed unchanged on the
package as it was before the chain moved there, which is what makes it a characterisation."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NOISE_DB = 15.0
N_PAYLOAD = 12_000
CONFIGS = [(w, il, outer, False) for w in ("csi", "noise", "noise2d") for il in (False, True) for outer in (None, (4, 2))] \
    + [("csi", il, outer, True) for il in (False, True) for outer in (None, (4, 2))]
IDS = [f"{w}{'-fused' if f else ''}-{'interleaved' if il else 'plain'}-{'outer42' if o else 'no_outer'}" for w, il, o, f in CONFIGS]


def _np(t):
    return t.cpu().numpy()


def _receiver(interleave, outer, weighting="csi", fused=False):
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A3", encoding="QCLDPC-1/2", no_pilots=4, packet_length=12)
    rx.interleave, rx.outer_code, rx.llr_weighting, rx.fused_llr = interleave, outer, weighting, fused
    return rx


@functools.lru_cache(maxsize=None)
def _stream(interleave, outer):
    """(payload, noisy stream) of one transmit side; shared by the weightings, never modified."""
    payload = np.random.default_rng(2026).integers(0, 2, size=N_PAYLOAD)
    tx = _receiver(interleave, outer)
    np.random.seed(17)
    sig = np.concatenate([np.zeros(2000), tx.transmit(payload), np.zeros(2000)])
    rms = np.sqrt(np.mean(sig[2000:-2000] ** 2))
    noisy = sig + np.random.default_rng(5).normal(0, rms / 10 ** (NOISE_DB / 20), sig.shape)
    return payload, noisy


def _outer_by_hand(rx, code, dec, iters, outer):
    """dec [n_cw, k], iters [n_cw] (device) -> (message bits, iters and statuses the report is made of), NumPy."""
    from gf3_audio_modem_amd.outer import OuterRS, transmitted_index
    if outer is None:
        return _np(dec).reshape(-1), _np(iters), np.zeros(0, dtype=np.int32)
    G, R = outer
    NG = dec.shape[0] // (G + R)
    rows = NG * (G + R)
    fixed, status = OuterRS(G, R, code.k).recover(dec[:rows].clone(), iters[:rows])
    fixed = _np(fixed)
    msg = np.concatenate([fixed[transmitted_index(g, t, NG)] for g in range(NG) for t in range(G)])
    return msg, _np(iters)[:rows], _np(status)


def _report_by_hand(iters, status):
    failed = np.flatnonzero(iters < 0)
    return {"codewords": len(iters), "inner_failed": len(failed), "recovered": int(status[status > 0].sum()),
            "groups_failed": int((status < 0).sum()), "failed_codewords": failed}


def _assert_report(rep, want):
    assert set(rep) == set(want)
    for k, v in want.items():
        assert np.array_equal(rep[k], v), (k, rep[k], v)


def _soft_chain_by_hand(rx, noisy, weighting, interleave, outer, fused):
    from gf3_audio_modem_amd import QCLDPC
    eng = rx._engine(noisy.dtype)
    x = eng._samples(noisy)
    starts = (eng.sync_stream(x) + 2)[:-1]
    snr = snr_s = None
    if fused:
        o = eng.demod_frames_llr(x, starts, weight="csi", want=("Hs", "He", "slope"))
        llr = o["llr"]
    else:
        o = eng.demod_frames(x, starts, want=("eq", "Hs", "He", "slope"))
        if weighting == "csi":
            llr = eng.soft_demap_csi(o["eq"], o["Hs"], o["He"])
        else:
            if weighting == "noise":
                var = eng.noise_estimate(o["eq"])
                llr = eng.soft_demap_nw(o["eq"], var)
            else:
                var, var_s = eng.noise_estimate2(o["eq"])
                llr = eng.soft_demap_nw2(o["eq"], var, var_s)
            # the SNR report: 10 log10(Es / v') with the demapper's floor (device arithmetic, as receive() does it)
            es = float(np.mean(np.abs(rx._tables()[0]) ** 2))
            floor = 1e-6 * var.mean(dim=1, keepdim=True)
            snr = _np(10.0 * torch.log10(es / torch.maximum(var, floor)))
            if weighting == "noise2d":
                snr_s = _np(10.0 * torch.log10(es / torch.maximum(var_s, floor)))
    if interleave:
        llr = eng.interleave(llr, inverse=True)
    code = QCLDPC("1/2")
    n_cw = llr.numel() // code.n
    dec, iters = code.decode(llr[: n_cw * code.n], max_iter=rx.ldpc_max_iter, want_iters=True)
    msg, its, status = _outer_by_hand(rx, code, dec, iters, outer)
    return dict(bits=msg.astype(np.int64), Hs0=_np(o["Hs"])[0], He0=_np(o["He"])[0], slope=_np(o["slope"]),
                report=_report_by_hand(its, status), snr=snr, snr_s=snr_s, iters=its, n_cw=n_cw)


@pytest.mark.parametrize("weighting,interleave,outer,fused", CONFIGS, ids=IDS)
def test_receive_is_the_chain_written_out_by_hand(weighting, interleave, outer, fused, capsys):
    payload, noisy = _stream(interleave, outer)
    rx = _receiver(interleave, outer, weighting, fused)
    bits, Hs0, He0 = rx.receive(noisy)
    want = _soft_chain_by_hand(_receiver(interleave, outer, weighting, fused), noisy, weighting, interleave, outer, fused)
    capsys.readouterr()
    assert want["n_cw"] == 28 and rx.no_packets == 2
    assert bits.dtype == np.int64 and np.array_equal(bits, want["bits"])
    assert len(bits) == (16 * 768 if outer else 28 * 768)
    assert np.array_equal(Hs0, want["Hs0"]) and np.array_equal(He0, want["He0"])
    assert np.array_equal(rx._last_slope, want["slope"])
    _assert_report(rx.last_decode_report, want["report"])
    assert rx.last_decode_report["codewords"] == (24 if outer else 28)
    if weighting == "csi":
        assert rx.last_snr_db is None and rx.last_symbol_snr_db is None
    else:
        assert rx.last_snr_db.shape == (2, 900) and np.array_equal(rx.last_snr_db, want["snr"])
        if weighting == "noise2d":
            assert rx.last_symbol_snr_db.shape == (2, 12) and np.array_equal(rx.last_symbol_snr_db, want["snr_s"])
        else:
            assert rx.last_symbol_snr_db is None
    # against vacuity: the payload is back, and the decoder had work to do on the message's codewords
    assert np.array_equal(bits[:N_PAYLOAD], payload)
    message = want["iters"][: 24 if outer else 16]
    print("iterations on the message's codewords:", message.tolist())
    assert (np.abs(message) > 1).any(), message


def test_decode_is_the_hard_chain_written_out_by_hand():
    """decode() on hard bits (noise2d, interleaver, (4, 2)): codewords 5 .. 8 (4 = NG consecutive) replaced by coin flips,
    so each group loses one member and the outer code rewrites it."""
    from gf3_audio_modem_amd import QCLDPC
    payload, _ = _stream(True, (4, 2))
    rx = _receiver(True, (4, 2), "noise2d")
    eng = rx._engine()
    np.random.seed(17)
    coded = np.asarray(rx.encode(payload))
    plain = _np(eng.interleave(torch.from_numpy(coded.astype(np.uint8)), inverse=True))
    plain[5 * 1536: 9 * 1536] = np.random.default_rng(3).integers(0, 2, size=4 * 1536)
    hurt = _np(eng.interleave(torch.from_numpy(plain), inverse=False))
    got = rx.decode(hurt)
    # by hand: de-interleave, +-1 LLRs of the whole codewords, decode, recover, regroup
    code = QCLDPC("1/2")
    b = _np(eng.interleave(torch.from_numpy(hurt), inverse=True))
    n_cw = len(b) // code.n
    llr = torch.from_numpy(1.0 - 2.0 * b[: n_cw * code.n].astype(np.float32))
    dec, iters = code.decode(llr, max_iter=rx.ldpc_max_iter, want_iters=True)
    msg, its, status = _outer_by_hand(rx, code, dec, iters, (4, 2))
    assert got.dtype == np.int64 and np.array_equal(got, msg.astype(np.int64))
    _assert_report(rx.last_decode_report, _report_by_hand(its, status))
    assert rx.last_decode_report["failed_codewords"].tolist() == [5, 6, 7, 8] and rx.last_decode_report["recovered"] == 4
    assert np.array_equal(got[:N_PAYLOAD], payload) and len(got) == 16 * 768
