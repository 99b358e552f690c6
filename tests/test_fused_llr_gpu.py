"""gf3_demod_frames_llr (MODE_SOFT of the fused demodulator: samples -> weighted max-log LLRs in one launch) against the
staged path it replaces -- demod_frames(want eq, Hs, He) + soft_demap_csi / soft_demap -- on every soft-decision case of
tests/tables.py, in the one-launch and the two-phase form.

Tolerance (derived, not measured): |fused - ref| <= 2^-22 |ref| + 1e-9 max_packet |ref|.  The staged CSI path rounds to
float32 twice and the fused path once (<= 1.5 x 2^-23 relative); between demodulator forms eq agrees to 1e-12 and the LLR
is Lipschitz in eq with a constant of a few table spans times the weight.

GF3_FUSED_LLR_PARITY_OUT=<file>: the parity test records the largest realised |delta| / tolerance per case there
(the place for such a record is profiles/fused_llr_parity.json)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import tables as T
from tests.util import engine_for

pytestmark = pytest.mark.gpu
SOFT_CASES = [i for i, c in enumerate(T.CASES) if c[0] in T.SOFT_TABLES]
SOFT_IDS = [T.CASE_IDS[i] for i in SOFT_CASES]
WANT = ("Hs", "He", "slope")
_RECORD = {}


def _np(t):
    return t.cpu().numpy()


def _tol(ref, F):
    r = np.abs(ref).reshape(F, -1)
    return (2.0 ** -22 * r + 1e-9 * r.max(axis=1, keepdims=True)).reshape(-1)


@functools.lru_cache(maxsize=None)
def _extra_case():
    """64-QAM on every carrier of N = 1024: C mu = 3066 floats per symbol do not fit the FFT buffer (9216 B), so the
    owners store their LLRs directly -- the one path no row of tables.CASES reaches.  Built as tables.demod_case builds."""
    p = T.params_for("qam64", 1024, T.all_reversed(511), P=2, D=3)
    rs = np.random.RandomState(77)
    F = 2
    payload = T.existing_labels_payload(rs, p, F * p.D * p.C)
    gaps = rs.randint(0, 200, F)
    r = orc.tx_stream(payload, rs.choice(T.QPSK_FILL, size=p.K - p.C), p, gaps=gaps, lead=30, tail=60)
    r = np.convolve(r, T.ECHO)[: len(r)]
    r = r + T.NOISE_REL * np.sqrt(np.mean(r * r)) * rs.randn(len(r))
    starts = 30 + np.cumsum(gaps) + np.arange(F) * p.frame_len + p.Lc
    return p, r, starts, "float64"


def _inputs(i):
    if i < 0:
        return _extra_case()
    p, x, starts, _, _ = T.demod_case(i)
    return p, x, starts, T.CASES[i][6]


@functools.lru_cache(maxsize=None)
def _runs(i):
    """Case i through the staged path and the fused call, both forms, both weights (host arrays; computed once)."""
    p, x, starts, storage = _inputs(i)
    eng = engine_for(p, in_dtype=getattr(torch, storage))
    xd = torch.from_numpy(x).cuda()
    F = len(starts)
    out = dict(p=p, F=F, plan=eng.demod_plan(F, split=True))
    for form in (False, True):
        o = eng.demod_frames(xd, starts, want=("eq",) + WANT, split=form)
        st = {k: _np(o[k]) for k in WANT}
        st["bits"] = _np(eng.unpack_bits(o["bits"]))
        if not form:                                       # the references: existing code on the one-launch dumps
            out["ref_csi"] = _np(eng.soft_demap_csi(o["eq"], o["Hs"], o["He"]))
            out["ref_none"] = _np(eng.soft_demap(o["eq"], 1.0)).reshape(-1)
        out["staged", form] = st
        for w in ("csi", "none"):
            f = eng.demod_frames_llr(xd, starts, weight=w, want=WANT, split=form)
            out["fused", form, w] = {k: _np(v) for k, v in f.items()}
    eng.close()
    return out


def _record(name, worst):
    path = os.environ.get("GF3_FUSED_LLR_PARITY_OUT")
    _RECORD[name] = worst
    if path:
        with open(path, "w") as fh:
            json.dump({"tolerance": "2^-22 |ref| + 1e-9 max_packet |ref|", "worst_delta_over_tolerance": _RECORD}, fh, indent=1)


# ---- 1. parity with the staged path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("i", SOFT_CASES + [-1], ids=SOFT_IDS + ["qam64-all_reversed-1024-direct-stores"])
def test_parity_with_the_staged_path(i):
    r = _runs(i)
    worst, bad = {}, []
    for form in (False, True):
        for w in ("csi", "none"):
            ref = r["ref_" + w]
            got = r["fused", form, w]["llr"]
            assert got.shape == ref.shape and got.dtype == np.float32
            ratio = float((np.abs(got.astype(np.float64) - ref) / _tol(ref, r["F"])).max())
            key = f"{'two-phase' if form else 'one-launch'}/{w}"
            worst[key] = ratio
            print(f"  {key}: max |delta| / tolerance = {ratio:.3g}")
            if not ratio <= 1.0:
                bad.append(key)
        for k in WANT:                                     # the channel state: the same values in the same form, bit for bit
            for w in ("csi", "none"):
                assert np.array_equal(r["fused", form, w][k], r["staged", form][k]), (form, w, k)
    _record("extra" if i < 0 else T.CASE_IDS[i], worst)
    assert not bad, (bad, worst)


# ---- 2. signs are the hard decisions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", SOFT_CASES, ids=SOFT_IDS)
def test_signs_are_the_hard_decisions(i):
    r = _runs(i)
    ref = r["ref_csi"]
    sure = np.abs(ref) > _tol(ref, r["F"])                # (the condition is checked on the staged LLRs)
    assert (~sure).mean() <= 1e-3
    for form in (False, True):
        bits = r["staged", form]["bits"].astype(bool)
        assert np.array_equal((r["fused", form, "csi"]["llr"] < 0)[sure], bits[sure]), form


# ---- 3. the two-phase form has no seam ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["psk8-descending-4096-P2-D40-float64", "qpsk_ref-single_top-2048-P2-D70-float64",
                                  "bpsk-single_top-1024-P2-D70-float64"])
def test_two_phase_form_has_no_seam(name):
    i = T.CASE_IDS.index(name)
    r = _runs(i)
    p = r["p"]
    assert r["plan"]["split"] and r["plan"]["chunks"] >= 2, r["plan"]
    for w in ("csi", "none"):
        one, two = r["fused", False, w]["llr"], r["fused", True, w]["llr"]
        assert (np.abs(two.astype(np.float64) - one) <= _tol(one.astype(np.float64), r["F"])).all(), w
        rows = two.reshape(r["F"] * p.D, p.C * p.mu)
        assert (rows != 0).any(axis=1).all(), (w, np.flatnonzero(~(rows != 0).any(axis=1)))     # no symbol left zero at a chunk boundary


# ---- 4. ragged frame --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [False, True], ids=["one-launch", "two-phase"])
def test_ragged_frame_is_a_row_of_positive_zeros(form):
    p, x, starts, _, _ = T.demod_case(0)                   # N = 1024
    assert p.N == 1024 and len(starts) == 2
    eng = engine_for(p)
    xd = torch.from_numpy(x).cuda()
    three = np.concatenate([starts, [len(x) - p.frame_len // 2]])
    n = p.D * p.C * p.mu
    out = torch.full((3 * n,), float("nan"), dtype=torch.float32, device="cuda")
    o = eng.demod_frames_llr(xd, three, want=("status",), split=form, out=out)
    assert o["llr"] is out
    got = _np(out)
    assert int(_np(o["status"])[0]) & 1
    assert np.array_equal(got[2 * n:].view(np.int32), np.zeros(n, np.int32))       # +0.0f: value and sign bit
    two = eng.demod_frames_llr(xd, starts, want=("status",), split=form)
    assert int(_np(two["status"])[0]) == 0
    assert np.array_equal(got[: 2 * n].view(np.int32), _np(two["llr"]).view(np.int32))
    assert np.isfinite(got).all()
    eng.close()


# ---- 5. arguments --------------------------------------------------------------------------------------------------------
def test_arguments():
    from gf3_audio_modem_amd.engine import Gf3Error
    p, x, starts, _, _ = T.demod_case(0)
    eng = engine_for(p)
    xd = torch.from_numpy(x).cuda()
    with pytest.raises(Gf3Error, match="weight"):
        eng.demod_frames_llr(xd, starts, weight=2)
    with pytest.raises(ValueError, match="weight"):
        eng.demod_frames_llr(xd, starts, weight="snr")
    n = len(starts) * p.D * p.C * p.mu
    for bad in (torch.empty(n + 1, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"),
                torch.empty(2 * n, dtype=torch.float32, device="cuda")[::2]):
        with pytest.raises(ValueError, match="out must be"):
            eng.demod_frames_llr(xd, starts, out=bad)
    empty = eng.demod_frames_llr(xd, np.zeros(0, np.int64), want=("Hs", "status"))
    assert empty["llr"].numel() == 0 and empty["llr"].dtype == torch.float32 and tuple(empty["Hs"].shape) == (0, p.K)
    eng.close()


def test_tri3_is_treated_as_soft_demap_treats_it():
    """gf3_soft_demap applies no condition on the table: tri3 (3 points on 2 bits) gets its max-log LLRs there, and so it
    does here, to the tolerance of the parity test."""
    i = T.CASE_IDS.index("tri3-two_bands-1024-P2-D3-float64")
    p, x, starts, _, _ = T.demod_case(i)
    eng = engine_for(p)
    xd = torch.from_numpy(x).cuda()
    o = eng.demod_frames(xd, starts, want=("eq", "Hs", "He"), split=False)
    ref = _np(eng.soft_demap_csi(o["eq"], o["Hs"], o["He"]))          # (accepted: the call this one mirrors)
    for form in (False, True):
        got = _np(eng.demod_frames_llr(xd, starts, split=form)["llr"])
        assert (np.abs(got.astype(np.float64) - ref) <= _tol(ref, len(starts))).all(), form
    eng.close()


# ---- 6. two calls, identical bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [False, True], ids=["one-launch", "two-phase"])
def test_two_calls_give_identical_bits(form):
    i = T.CASE_IDS.index("qam64-shuffled-4096-P2-D3-int16")
    p, x, starts, _, _ = T.demod_case(i)
    eng = engine_for(p, in_dtype=torch.int16)
    xd = torch.from_numpy(x).cuda()
    a = _np(eng.demod_frames_llr(xd, starts, split=form)["llr"])
    b = _np(eng.demod_frames_llr(xd, starts, split=form)["llr"])
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    eng.close()


# ---- 7. end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleave", [False, True], ids=["plain", "interleaved"])
def test_receive_with_fused_llr_returns_the_payload(interleave, capsys):
    """The AWGN scenario of tests/test_ldpc_gpu.py (mode A2, "QCLDPC-1/2", noise 7 dB below the signal; its stream builder
    is not exposed, the construction is restated): fused_llr = True returns the payload, prints and returns what the
    staged path does."""
    from gf3_audio_modem_amd.OFDM import receiver
    rng = np.random.default_rng(2026)
    payload = rng.integers(0, 2, size=150_000)
    tx = receiver("A2", encoding="QCLDPC-1/2")
    tx.interleave = interleave
    np.random.seed(17)
    sig = tx.transmit(payload)
    sig = np.concatenate([np.zeros(2000), sig, np.zeros(2000)])
    noisy = sig + rng.normal(0, np.sqrt(np.mean(sig[2000:-2000] ** 2) / 10 ** 0.7), sig.shape)
    capsys.readouterr()
    res = {}
    for fused in (False, True):
        rx = receiver("A2", encoding="QCLDPC-1/2")
        rx.interleave = interleave
        rx.fused_llr = fused
        res[fused] = rx.receive(noisy) + (capsys.readouterr().out,)
    out, Hs0, He0, text = res[True]
    assert np.array_equal(out[: len(payload)], payload)
    # the decoder's output on the payload's codewords is the staged path's; behind them the packet carries the
    # transmitter's random fill, which is no codeword: what the decoder makes of it hangs on the last bit of every LLR
    # and is nobody's result
    whole = -(-len(payload) // 768) * 768
    assert len(out) == len(res[False][0]) and np.array_equal(out[:whole], res[False][0][:whole])
    assert not out[len(payload): whole].any()
    assert np.array_equal(Hs0, res[False][1]) and np.array_equal(He0, res[False][2])
    assert text == res[False][3] and "Number of received bits" in text
