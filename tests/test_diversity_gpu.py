"""Receive diversity on the GPU: gf3_combine_branches against the NumPy restatement (tests/diversity_ref.py) on every
demapper path, its single-branch forms, planted weights, edge inputs and argument checks, and receive_diversity end to
end on the two-microphone scenario of DESIGN §12 (tests/test_diversity_cpu.py holds its CPU form)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import diversity_ref as DR
from tests import noise_ref as NR
from tests import tables as T

pytestmark = pytest.mark.gpu
LEVEL_DB = 13.0                                            # the level tests/test_diversity_cpu.py settled on


def engine_of(p, **kw):
    from gf3_audio_modem_amd import Engine, RxConfig
    return Engine(RxConfig(N=p.N, CP=p.CP, P=p.P, D=p.D, data_bins=p.data_carriers, const_points=p.const_points,
                           const_bits=p.const_bits, known_bits=p.known_bits, in_dtype=torch.float64,
                           fit_lo=p.fit_lo, fit_hi=p.fit_hi, **kw))


def small_params(pts, bits, D=7, carriers=None):
    """test_noise_gpu.test_other_tables' geometry: C = 395 is no multiple of 64 or 256 (two tiles, the second partial)"""
    bits = np.asarray(bits).astype(np.int64)
    return orc.RxParams(N=1024, CP=0, P=1, D=D, lo=5, hi=400, carriers=carriers, const_points=np.asarray(pts), const_bits=bits,
                        known_bits=np.zeros(511 * bits.shape[1], np.uint8), fit_lo=10, fit_hi=100)


def branches(p, F, B, seed):
    """B branches of the same seeded symbols with per-branch, per-carrier noise; random Hs / He [F, K] per branch"""
    rng = np.random.default_rng(seed)
    pts = p.const_points
    idx = rng.integers(0, len(pts), size=(F * p.D, p.C))
    eqs, Hs, He = [], [], []
    for _ in range(B):
        sig = 0.02 + 0.1 * rng.random(p.C)
        eqs.append(pts[idx] + (rng.normal(size=idx.shape) + 1j * rng.normal(size=idx.shape)) * sig)
        Hs.append((rng.normal(size=(F, p.K)) + 1j * rng.normal(size=(F, p.K))) * 0.7)
        He.append(Hs[-1] * (1 + 0.3 * rng.normal(size=(F, p.K))) * np.exp(0.2j * rng.normal(size=(F, p.K))))
    return idx, eqs, Hs, He


def same_bytes(a, b):
    return all(np.array_equal(a[k].cpu().numpy().reshape(-1).view(np.uint8), b[k].cpu().numpy().reshape(-1).view(np.uint8)) for k in a)


def check_against_restatement(p, eng, eqs, Hs=None, He=None, var=None):
    """One call with every output against the restatement, the LLR signs against the plain demapper on the combined
    symbols, and a second call's bytes -> the outputs as NumPy arrays"""
    want = ("eq", "w", "llr")
    o = eng.combine_branches(eqs, Hs=Hs, He=He, var=var, want=want)
    if var is None:
        z, W, llr = DR.combine_csi(eqs, Hs, He, p.data_carriers, p.P, p.D, p.const_points, p.const_bits)
    else:
        z, W, llr = DR.combine_noise(eqs, var, p.D, p.const_points, p.const_bits)
    got = {k: o[k].cpu().numpy() for k in want}
    assert got["eq"].dtype == np.complex128 and got["w"].dtype == np.float64 and got["llr"].dtype == np.float32
    assert got["eq"].shape == got["w"].shape == z.shape and got["llr"].shape == llr.shape
    np.testing.assert_allclose(got["eq"], z, rtol=1e-12)
    np.testing.assert_allclose(got["w"], W, rtol=1e-12)
    np.testing.assert_allclose(got["llr"], llr, rtol=1e-6, atol=1e-9 * np.abs(llr).max())
    plain = eng.soft_demap(o["eq"], 1.0).cpu().numpy().reshape(-1)
    live = np.repeat(got["w"].reshape(-1) > 0, p.mu)
    assert np.array_equal(np.sign(got["llr"])[live], np.sign(plain)[live])
    assert not got["llr"][~live].any() and not np.signbit(got["llr"][~live]).any()
    assert same_bytes(o, eng.combine_branches(eqs, Hs=Hs, He=He, var=var, want=want))
    return got


def table_of(kind):
    if kind == "qam16_reversed_labels":
        pts, bits = orc.square_qam_table(4)
        return pts, bits[:, ::-1].copy()
    if kind == "ring8":
        return T.TABLES["ring8"]
    return {"qpsk": orc.qpsk_table, "qam4_binary": lambda: orc.square_qam_table(2), "qam16": lambda: orc.square_qam_table(4), "qam64": lambda: orc.square_qam_table(6)}[kind]()


@pytest.mark.parametrize("kind,carriers", [("qpsk", None), ("qam16", None), ("qam64", None), ("qam16_reversed_labels", None),
                                           ("ring8", None), ("qam16", "shuffled"), ("qam4_binary", None)])
def test_kernel_matches_restatement(kind, carriers):
    """B = 1 .. 4 in both modes: the three straight-line grid kernels (HI = 1: the binary-indexed 4-point grid, not the
    reference's QPSK, whose first label bit belongs to the Q axis and which takes the table-generic path), a grid with
    reversed labels and a table that is no grid (the table-generic path), and 16-QAM on a scattered carrier map (the csi
    weights go through the carriers' bins)."""
    pts, bits = table_of(kind)
    p = small_params(pts, bits, carriers=None if carriers is None else T.MAPS[carriers](511))
    eng = engine_of(p)
    F = 5
    _, eqs, Hs, He = branches(p, F, 4, len(kind))
    var = [NR.noise_estimate(e, p.const_points, p.D) for e in eqs]
    for B in (1, 2, 3, 4):
        check_against_restatement(p, eng, eqs[:B], Hs=Hs[:B], He=He[:B])
        check_against_restatement(p, eng, eqs[:B], var=var[:B])
        # the estimate the façade feeds it: the engine's own
        dev = [eng.noise_estimate(e) for e in eqs[:B]]
        o = eng.combine_branches(eqs[:B], var=dev, want=("w",))["w"].cpu().numpy()
        np.testing.assert_allclose(o, DR.combine_noise(eqs[:B], var[:B], p.D, p.const_points, p.const_bits)[1], rtol=1e-11)


@pytest.mark.parametrize("kind", ["qpsk", "qam64", "ring8"])
def test_one_branch_is_the_single_branch_demapper(kind):
    pts, bits = table_of(kind)
    p = small_params(pts, bits)
    eng = engine_of(p)
    _, eqs, Hs, He = branches(p, 5, 1, 3)
    var = eng.noise_estimate(eqs[0])
    for kw, single in ((dict(var=[var]), eng.soft_demap_nw(eqs[0], var)), (dict(Hs=Hs, He=He), eng.soft_demap_csi(eqs[0], Hs[0], He[0]))):
        o = eng.combine_branches(eqs, **kw)
        ref = single.cpu().numpy()
        np.testing.assert_allclose(o["llr"].cpu().numpy(), ref, rtol=1e-6, atol=1e-9 * np.abs(ref).max())
        np.testing.assert_allclose(o["eq"].cpu().numpy(), eqs[0], rtol=1e-12)
        assert sorted(o) == ["eq", "llr"]


def test_planted_weights():
    """Two branches carry the same clean symbols; branch 1's carriers in the upper half get noise of 9x the variance.  The
    noise weights there are 1/v0 + 1/(9 v0) within the estimate's own value (the restatement on the measured variances;
    chi-square with 2 D degrees of freedom: relative standard deviation 1 / sqrt(D), 5 sigma), and swapping the branches
    changes the result by rounding only."""
    pts, bits = orc.qpsk_table()
    p = small_params(pts, bits, D=64)
    eng = engine_of(p)
    rng = np.random.default_rng(12)
    F, v0 = 2, 0.002
    idx = rng.integers(0, 4, size=(F * p.D, p.C))
    n0, n1 = (rng.normal(size=(2,) + idx.shape) + 1j * rng.normal(size=(2,) + idx.shape)) * np.sqrt(v0 / 2)
    n1[:, p.C // 2:] *= 3.0
    eqs = [pts[idx] + n0, pts[idx] + n1]
    var = [eng.noise_estimate(e) for e in eqs]
    host = [v.cpu().numpy() for v in var]
    got = check_against_restatement(p, eng, eqs, var=host)
    hi = got["w"].reshape(F, p.D, p.C)[:, 0, p.C // 2:]
    assert np.abs(hi / (1 / v0 + 1 / (9 * v0)) - 1.0).max() < 5.0 / np.sqrt(p.D)
    lo = got["w"].reshape(F, p.D, p.C)[:, 0, : p.C // 2]
    assert np.abs(lo / (2 / v0) - 1.0).max() < 5.0 / np.sqrt(p.D)
    swapped = eng.combine_branches(eqs[::-1], var=var[::-1], want=("eq", "w", "llr"))
    np.testing.assert_allclose(swapped["eq"].cpu().numpy(), got["eq"], rtol=1e-12)
    np.testing.assert_allclose(swapped["w"].cpu().numpy(), got["w"], rtol=1e-12)
    np.testing.assert_allclose(swapped["llr"].cpu().numpy(), got["llr"], rtol=1e-6, atol=1e-9 * np.abs(got["llr"]).max())
    _, _, Hs, He = branches(p, F, 2, 5)
    a = check_against_restatement(p, eng, eqs, Hs=Hs, He=He)
    b = eng.combine_branches(eqs[::-1], Hs=Hs[::-1], He=He[::-1])
    np.testing.assert_allclose(b["eq"].cpu().numpy(), a["eq"], rtol=1e-12)
    np.testing.assert_allclose(b["llr"].cpu().numpy(), a["llr"], rtol=1e-6, atol=1e-9 * np.abs(a["llr"]).max())


def test_edge_inputs():
    pts, bits = orc.qpsk_table()
    p = small_params(pts, bits)
    eng = engine_of(p)
    F, D, Cn = 4, p.D, p.C
    _, eqs, Hs, He = branches(p, F, 2, 21)
    eqs = [e.copy() for e in eqs]
    eqs[0][3, 17] = complex(np.nan, 0.0)                   # one branch: the other comes through alone
    eqs[1][4, 300] = complex(1.0, np.inf)
    for e in eqs:                                          # every branch: nothing is left
        e[5, 258] = complex(np.nan, np.nan)
    eqs[0][6, 2], eqs[1][6, 2] = complex(0.0, -np.inf), complex(np.nan, 1.0)
    var = [NR.noise_estimate(e, pts, D) for e in eqs]      # (NaN on the carriers above, so packet 0's vbar is NaN: weights 1)
    var[0][1, 9] = np.inf                                  # a non-finite variance on one carrier of one branch
    var[1][2] = 0.0                                        # a branch with all-zero variance in packet 2: it dominates
    var[0][3] = var[1][3] = 0.0                            # vbar = 0 in packet 3: weights 1
    Hs[1][1, p.data_carriers[40] - 1] = complex(np.inf, 0.0)
    He[0][2, p.data_carriers[41] - 1] = complex(0.0, np.nan)
    for kw in (dict(var=var), dict(Hs=Hs, He=He)):
        got = check_against_restatement(p, eng, eqs, **kw)
        z, W, llr = got["eq"], got["w"], got["llr"].reshape(F * D, Cn, 2)
        assert np.isfinite(z).all() and np.isfinite(W).all() and np.isfinite(llr).all()
        np.testing.assert_allclose(z[3, 17], eqs[1][3, 17], rtol=1e-12)
        np.testing.assert_allclose(z[4, 300], eqs[0][4, 300], rtol=1e-12)
        for at in ((5, 258), (6, 2)):
            assert z[at] == 0 and W[at] == 0 and not llr[at].any() and not np.signbit(llr[at]).any()
    got = check_against_restatement(p, eng, eqs, var=var)
    W = got["w"].reshape(F, D, Cn)
    assert W[0, 0, 5] == 2.0 and W[0, 3, 17] == 1.0        # packet 0: vbar is NaN -> weights 1; the NaN symbol's branch drops out
    assert W[1, 0, 9] == 1.0                               # packet 1: vbar is Inf -> weights 1, the Inf variance's branch 0
    np.testing.assert_allclose(got["eq"][2 * D: 3 * D], eqs[1][2 * D: 3 * D], rtol=1e-4)       # packet 2: branch 1 at 1e6 / vbar
    assert (W[2] > 1e5 / var[0][2].mean()).all()
    assert np.array_equal(W[3], np.full((D, Cn), 2.0))     # packet 3: vbar = 0 -> weights 1
    got = check_against_restatement(p, eng, eqs, Hs=Hs, He=He)
    np.testing.assert_allclose(got["eq"].reshape(F, D, Cn)[1, :, 40], eqs[0].reshape(F, D, Cn)[1, :, 40], rtol=1e-12)
    np.testing.assert_allclose(got["eq"].reshape(F, D, Cn)[2, :, 41], eqs[1].reshape(F, D, Cn)[2, :, 41], rtol=1e-12)


@pytest.mark.parametrize("D,carriers", [(1, None), (3, [7]), (1, [511])])
def test_smallest_geometries(D, carriers):
    pts, bits = orc.square_qam_table(4)
    p = small_params(pts, bits, D=D, carriers=carriers)
    eng = engine_of(p)
    _, eqs, Hs, He = branches(p, 3, 3, D)
    check_against_restatement(p, eng, eqs, Hs=Hs, He=He)
    check_against_restatement(p, eng, eqs, var=[NR.noise_estimate(e, p.const_points, p.D) for e in eqs])
    # F = 0: nothing to do, empty outputs
    o = eng.combine_branches([np.zeros((0, p.C), complex)] * 2, var=[np.zeros((0, p.C))] * 2, want=("eq", "w", "llr"))
    assert [o[k].numel() for k in ("eq", "w", "llr")] == [0, 0, 0]


def test_argument_checks():
    from gf3_audio_modem_amd import _lib
    pts, bits = orc.qpsk_table()
    p = small_params(pts, bits)
    eng = engine_of(p)
    F = 2
    _, eqs, Hs, He = branches(p, F, 2, 8)
    var = [NR.noise_estimate(e, pts, p.D) for e in eqs]
    dev = [eng._dev(e) for e in eqs]
    n = F * p.D * p.C
    bad = [dict(var=var, Hs=Hs, He=He), dict(), dict(Hs=Hs), dict(He=He, var=var), dict(var=var[:1]), dict(Hs=Hs, He=He[:1]),
           dict(var=[var[0], var[1][:1]]), dict(Hs=[Hs[0], Hs[1][:, :-1]], He=He), dict(var=var, want=()), dict(var=var, want=("eq", "bits")),
           dict(var=var, out={"eq": torch.empty(n - 1, dtype=torch.complex128, device="cuda")}),
           dict(var=var, out={"eq": torch.empty(n, dtype=torch.complex64, device="cuda")}),
           dict(var=var, out={"llr": torch.empty(n * 2, dtype=torch.float64, device="cuda")}),
           dict(var=var, out={"w": torch.empty(n, dtype=torch.float32, device="cuda")}),
           dict(var=var, out={"w": torch.empty(n, dtype=torch.float64, device="cuda")}, want=("eq",)),
           dict(var=var, out={"eq": dev[1]})]
    for kw in bad:
        with pytest.raises(ValueError, match="combine_branches"):
            eng.combine_branches(dev, **kw)
    for eqs_bad in ([], dev * 3, [dev[0], dev[1][: p.D]]):
        with pytest.raises(ValueError, match="combine_branches"):
            eng.combine_branches(eqs_bad, var=var)
    out = {"eq": torch.empty(n, dtype=torch.complex128, device="cuda"), "llr": torch.empty(2 * n, dtype=torch.float32, device="cuda")}
    o = eng.combine_branches(dev, var=var, out=out)
    assert o["eq"].data_ptr() == out["eq"].data_ptr() and o["llr"].data_ptr() == out["llr"].data_ptr()
    assert same_bytes(o, eng.combine_branches(dev, var=var))

    # the raw ABI
    lib = eng.lib
    dvar = [eng._dev(v, torch.float64) for v in var]
    dHs, dHe = [eng._dev(h) for h in Hs], [eng._dev(h) for h in He]
    tab = lambda xs: (C.c_void_p * len(xs))(*[None if x is None else x.data_ptr() for x in xs])
    q = _lib.ptr(out["eq"])
    E, V, S, G = tab(dev), tab(dvar), tab(dHs), tab(dHe)
    call = lambda *a: lib.gf3_combine_branches(*a, None)
    assert call(eng._h, 2, E, 1, None, None, V, 0, q, None, None) == 0       # F == 0: a no-op, whatever the pointers
    assert call(eng._h, 9, None, 7, None, None, None, 0, None, None, None) == 0
    cases = {"no context": (None, 2, E, 1, None, None, V, F, q, None, None), "B = 0": (eng._h, 0, E, 1, None, None, V, F, q, None, None),
             "B = 5": (eng._h, 5, E, 1, None, None, V, F, q, None, None), "no branches": (eng._h, 2, None, 1, None, None, V, F, q, None, None),
             "null branch": (eng._h, 2, tab([dev[0], None]), 1, None, None, V, F, q, None, None),
             "no var": (eng._h, 2, E, 1, S, G, None, F, q, None, None), "null var": (eng._h, 2, E, 1, None, None, tab([dvar[0], None]), F, q, None, None),
             "no Hs": (eng._h, 2, E, 0, None, G, V, F, q, None, None), "no He": (eng._h, 2, E, 0, S, None, V, F, q, None, None),
             "null He": (eng._h, 2, E, 0, S, tab([None, dHe[1]]), None, F, q, None, None),
             "no output": (eng._h, 2, E, 1, None, None, V, F, None, None, None), "F < 0": (eng._h, 2, E, 1, None, None, V, -1, q, None, None),
             "mode": (eng._h, 2, E, 2, S, G, V, F, q, None, None), "mode ": (eng._h, 2, E, -1, S, G, V, F, q, None, None),
             "aliased": (eng._h, 2, E, 1, None, None, V, F, _lib.ptr(dev[1]), None, None),
             "too many packets": (eng._h, 2, E, 1, None, None, V, 65536, q, None, None)}
    for text, args in cases.items():
        assert call(*args) == _lib.GF3_EINVAL, text
        assert b"gf3_combine_branches" in lib.gf3_last_error(None), text
    assert call(eng._h, 2, E, 0, S, G, None, F, q, None, None) == 0          # (csi: the variances are not read)
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------------------------------
def facade(encoding, **attrs):
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2", encoding=encoding, packet_length=20)
    for k, v in attrs.items():
        setattr(rx, k, v)
    return rx


@functools.lru_cache(maxsize=None)
def recordings(encoding, interleave=False):
    """One packet through `transmit` and the two rooms of the scenario, noise at the nominal level; both recordings cut to
    one length -> (payload, coded bits as sent, [branch 0, branch 1])"""
    rx = facade(encoding, interleave=interleave)
    n = 36 * 1280 if encoding != "None" else 20 * 2800
    payload = np.random.default_rng(3).integers(0, 2, size=n)
    np.random.seed(5)                                       # (the fill of the last packet, the filler of the unused carriers)
    coded = np.asarray(rx.encode(payload))
    np.random.seed(5)
    tx = rx.transmit(payload)
    clean = DR.two_paths(tx)
    m = min(len(b) for b in clean)
    return payload, coded, DR.add_noise([b[:m] for b in clean], tx, LEVEL_DB)


def oracle_params(rx):
    pts, bt = orc.qpsk_table()
    return orc.RxParams(N=4096, CP=224, P=20, D=20, lo=100, hi=1500, const_points=pts, const_bits=bt,
                        known_bits=np.asarray(rx.known_sequence, dtype=np.uint8))


def test_receive_diversity_decodes_what_neither_recording_does():
    from gf3_audio_modem_amd.ldpc import shift_table
    payload, coded, br = recordings("QCLDPC-5/6")
    rx = facade("QCLDPC-5/6")
    p = oracle_params(rx)
    pts, bt = p.const_points, p.const_bits
    # the restatement on these samples
    sh = shift_table("5/6")
    msg = payload.reshape(36, 1280).astype(np.uint8)
    outs = [orc.receive(b, p) for b in br]
    eqs = [o["eq"] for o in outs]
    vars_ = [NR.noise_estimate(e, pts, p.D) for e in eqs]
    alone = [DR.failed(sh, DR.single_llrs(o, "csi", p), msg) for o in outs]
    comb = [DR.failed(sh, DR.combine_csi(eqs, [o["Hs"] for o in outs], [o["He"] for o in outs], p.data_carriers, p.P, p.D, pts, bt)[2], msg),
            DR.failed(sh, DR.combine_noise(eqs, vars_, p.D, pts, bt)[2], msg)]
    print(f"restated: alone failed {alone}, combined failed {comb} (csi, noise)")
    assert min(alone) >= 1 and comb == [0, 0]
    # the GPU
    for b in br:
        bits, _, _ = rx.receive(b)
        assert not np.array_equal(bits[: len(payload)], payload) and rx.last_decode_report["inner_failed"] > 0
    for weighting in ("csi", "noise"):
        rx = facade("QCLDPC-5/6", llr_weighting=weighting)
        bits, Hs0, He0 = rx.receive_diversity(br)
        assert bits.dtype == np.int64 and np.array_equal(bits[: len(payload)], payload)
        assert rx.last_decode_report["inner_failed"] == 0 and rx.last_decode_report["codewords"] == 36
        np.testing.assert_allclose(Hs0, outs[0]["Hs"][0], rtol=1e-9, atol=1e-9 * np.abs(outs[0]["Hs"][0]).max())
        np.testing.assert_allclose(He0, outs[0]["He"][0], rtol=1e-9, atol=1e-9 * np.abs(outs[0]["He"][0]).max())
        st = rx.last_branch_starts
        assert st.dtype == np.int64 and st.shape == (2, 1) and st[1, 0] - st[0, 0] == DR.DELAY
        assert np.array_equal(st, np.array([o["starts"] for o in outs]))
        if weighting == "csi":
            assert rx.last_branch_snr_db is None
            continue
        assert rx.last_branch_snr_db.shape == (2, 1, p.C) and rx.last_snr_db.shape == (1, p.C)
        np.testing.assert_allclose(rx.last_branch_snr_db, DR.branch_snr_db(vars_, pts), rtol=0, atol=1e-6)
        np.testing.assert_allclose(rx.last_snr_db, DR.combined_snr_db(vars_, pts), rtol=0, atol=1e-6)
        assert (rx.last_snr_db[None] > rx.last_branch_snr_db).all()
    # a 2-D array of the same samples
    bits2, _, _ = rx.receive_diversity(np.stack(br))
    assert np.array_equal(bits2, bits)


def test_receive_diversity_uncoded_has_fewer_errors():
    payload, coded, br = recordings("None")
    rx = facade("None")
    p = oracle_params(rx)
    assert np.array_equal(coded, payload)
    single = []
    for b in br:
        bits, _, _ = rx.receive(b)
        single.append(int(np.sum(bits != payload)))
    bits, _, _ = rx.receive_diversity(br)
    errors = int(np.sum(bits != payload))
    print(f"bit errors: alone {single}, combined {errors} of {len(payload)}")
    assert bits.shape == payload.shape and errors < min(single)
    # the restatement's decisions on the oracle's symbols, wherever they are not within 1e-6 of a boundary
    outs = [orc.receive(b, p) for b in br]
    z = DR.combine_csi([o["eq"] for o in outs], [o["Hs"] for o in outs], [o["He"] for o in outs], p.data_carriers, p.P, p.D,
                       p.const_points, p.const_bits)[0]
    d = np.sort(np.abs(z[..., None] - p.const_points), axis=-1)
    clear = np.repeat((d[..., 1] - d[..., 0] > 1e-6).reshape(-1), p.mu)
    ref = p.const_bits[NR.decide(z, p.const_points)].reshape(-1)
    assert clear.mean() > 0.999 and np.array_equal(bits[clear], ref[clear])
    assert int(np.sum(bits[clear] != payload[clear])) == int(np.sum(ref[clear] != payload[clear]))
    # XOR whitening on both ends
    rx = facade("XOR")
    np.random.seed(5)
    tx = rx.transmit(payload)
    clean = DR.two_paths(tx)
    bits, _, _ = rx.receive_diversity(DR.add_noise(clean, tx, LEVEL_DB))
    assert int(np.sum(bits != payload)) < min(single)


def test_receive_diversity_with_the_interleaver():
    payload, _, br = recordings("QCLDPC-5/6", True)
    for weighting in ("csi", "noise"):
        rx = facade("QCLDPC-5/6", interleave=True, llr_weighting=weighting)
        bits, _, _ = rx.receive_diversity(br)
        assert np.array_equal(bits[: len(payload)], payload)


def test_receive_diversity_refuses_different_packet_counts():
    _, _, br = recordings("QCLDPC-5/6")
    rx = facade("QCLDPC-5/6")
    with pytest.raises(ValueError, match=r"different numbers of packets: \[1, 3\]"):
        rx.receive_diversity([br[0], np.concatenate([br[1], br[1]])])
