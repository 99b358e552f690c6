"""The two-speaker receive paths under coloured noise on the GPU: gf3_mimo_pilot_noise, gf3_joint_noise_weights,
gf3_mimo_detect_nw and gf3_stbc_detect_nw against the NumPy restatement (tests/joint_noise_ref.py), edge inputs, refusals,
and receive_mimo / receive_stbc under joint_weighting = "noise" end to end in the restatement's coloured noise
(tests/test_joint_noise_cpu.py holds the CPU form and what the feature is worth).  The guard-band rows of the four entries
are in tests/test_bounds_joint_noise_gpu.py.

Shapes: those of tests/test_mimo_gpu.py -- N = 1024, CP in {32, 64}, P in {4, 6}, D = 7 (6 for the space-time code), data
bins 5 .. 399 (C = 395: two 256-carrier tiles, the second partial), F = 3."""
import functools

import numpy as np
import pytest
import torch

from oracle import gf3_oracle as orc
from tests import diversity_ref as DR
from tests import joint_noise_ref as JR
from tests import mimo_ref as MR
from tests import stbc_ref as SR
from tests import tables as T
from tests.joint_checks import held_to_the_restatement as joint_held
from tests.test_mimo_gpu import LEAD, TAIL, detect_inputs, engine_of, quiet, same_bytes, small_params

pytestmark = pytest.mark.gpu
F3 = 3
PILOT_RTOL = 1e-12                                          # what tests/test_mimo_gpu.py holds mimo_pilots to


def engine_in(p, dtype):
    from gf3_audio_modem_amd import Engine, RxConfig
    return Engine(RxConfig(N=p.N, CP=p.CP, P=p.P, D=p.D, data_bins=p.data_carriers, const_points=p.const_points,
                           const_bits=p.const_bits, known_bits=p.known_bits, in_dtype=dtype, fit_lo=p.fit_lo, fit_hi=p.fit_hi))


# ---- gf3_mimo_pilot_noise ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pilot_case(CP, P):
    """Three packet pairs through the scenario's room with 1 % of noise, microphone 0 -> (p, samples, starts)"""
    p = small_params(CP, P)
    rng = np.random.default_rng(CP + P)
    bits = rng.integers(0, 2, size=2 * F3 * p.D * p.C * p.mu)
    r = MR.through(MR.tx_mimo(bits, rng.choice(T.QPSK_FILL, size=p.K - p.C), p, lead=100, tail=300))[0]
    r = r + 0.01 * np.sqrt(np.mean(r * r)) * rng.normal(size=len(r))
    starts = 100 + np.arange(F3) * p.frame_len + p.Lc + MR.LEAD - 16
    return p, r, starts.astype(np.int64)


def held_to_the_restatement(got, r, starts, H, p, what):
    """v against the restatement on the SAME estimates H, relative to v itself (a small difference of large numbers: with
    1 % of noise in the samples the residual is a hundredth of the terms it is the difference of)"""
    ref, _ = JR.pilot_noise(r, starts, H, p)
    print(f"{what}: worst relative deviation from the restatement {np.max(np.abs(got / ref - 1)):.2e}")
    np.testing.assert_allclose(got, ref, rtol=PILOT_RTOL)
    return ref


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("CP", [64, 32])
@pytest.mark.parametrize("P", [4, 6])
def test_pilot_noise_against_the_restatement(P, CP, dtype):
    p, r, starts = pilot_case(CP, P)
    if dtype == torch.float32:
        r = r.astype(np.float32)
    eng = engine_in(p, dtype)
    H, _ = eng.mimo_pilots(r, starts)
    var, status = eng.mimo_pilot_noise(r, starts, H)
    got, Hn = var.cpu().numpy(), H.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (F3, 2, p.K) and status.dtype == torch.int32
    assert status.cpu().numpy().tolist() == [0, 0, 0]
    ref = held_to_the_restatement(got, r, starts, Hn, p, f"P {P}, CP {CP}, {dtype}")
    if CP == 64:
        # it measures the noise that was added: 1 % of the recording's RMS per sample, N sigma^2 per bin, over |X| = 1.  (The
        # room's echoes outlast a prefix of 32 samples, and what they carry over from symbol to symbol is noise too.)
        sigma2 = 1e-4 * np.mean(np.asarray(r, dtype=np.float64) ** 2)
        assert abs(got.mean() / (p.N * sigma2) - 1.0) < 0.1 and abs(ref.mean() / (p.N * sigma2) - 1.0) < 0.1
    var2, status2 = eng.mimo_pilot_noise(r, starts, H)
    assert same_bytes(var, var2) and same_bytes(status, status2)
    # a packet cut off at either end: status 1 and NaN rows, the neighbours as they were
    L = p.M * p.S
    off = np.array([-1, starts[0], len(r) - L + 1, starts[1], len(r), starts[2], -2 ** 40, 2 ** 40], dtype=np.int64)
    Hc = np.full((8, 2, 2, p.K), complex(np.nan, np.nan))
    Hc[[1, 3, 5]] = Hn
    vc, sc = eng.mimo_pilot_noise(r, off, Hc)
    vc = vc.cpu().numpy()
    assert sc.cpu().numpy().tolist() == [1, 0, 1, 0, 1, 0, 1, 1]
    assert np.isnan(vc[[0, 2, 4, 6, 7]]).all() and np.array_equal(vc[[1, 3, 5]], got)
    # the last packet ending on the last sample
    ve, se = eng.mimo_pilot_noise(r[: starts[2] + L], starts, H)
    assert se.cpu().numpy().tolist() == [0, 0, 0] and np.array_equal(ve.cpu().numpy(), got)


@pytest.mark.parametrize("N", [2048, 4096, 8192])
def test_pilot_noise_at_the_other_transform_sizes(N):
    """One packet pair of 4 + 1 + 4 symbols per size (the kernel is instantiated per transform size), in float32 samples"""
    p = small_params(CP=32, P=4, D=1, N=N)
    rng = np.random.default_rng(N)
    bits = rng.integers(0, 2, size=2 * p.D * p.C * p.mu)
    r = MR.through(MR.tx_mimo(bits, rng.choice(T.QPSK_FILL, size=p.K - p.C), p, lead=10, tail=100))[1]
    r = (r + 0.01 * np.sqrt(np.mean(r * r)) * rng.normal(size=len(r))).astype(np.float32)
    starts = np.array([10 + p.Lc + MR.LEAD - 8])
    eng = engine_in(p, torch.float32)
    H, _ = eng.mimo_pilots(r, starts)
    var, status = eng.mimo_pilot_noise(r, starts, H)
    assert status.cpu().numpy().tolist() == [0]
    held_to_the_restatement(var.cpu().numpy(), r, starts, H.cpu().numpy(), p, f"N {N}")


def test_pilot_noise_refusals():
    x = np.zeros(40000)
    for P in (2, 3, 5):
        eng = engine_of(small_params(P=P))
        with pytest.raises(ValueError, match=rf"gf3_mimo_pilot_noise.*P >= 4 \(P={P}\)"):
            eng.mimo_pilot_noise(x, [0], np.zeros((1, 2, 2, 511), complex))
    eng = engine_of(small_params(P=4))
    with pytest.raises(ValueError, match="mimo_pilot_noise: H must be"):
        eng.mimo_pilot_noise(x, [0, 100], np.zeros((1, 2, 2, 511), complex))
    var, status = eng.mimo_pilot_noise(x, np.zeros(0, dtype=np.int64), np.zeros((0, 2, 2, 511), complex))
    assert var.shape == (0, 2, 511) and status.numel() == 0


# ---- gf3_joint_noise_weights ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["qpsk", "shuffled"])
def test_weights_are_the_combiners_rule_bit_for_bit(kind):
    """Packets: 0 ordinary, 1 with a NaN variance on one side of one carrier of one branch (w 0 there, and the packet's mean
    is not finite: 1 elsewhere), 2 all zero (1), 3 with an infinite variance (0 there, 1 elsewhere), 4 ordinary again with a
    NaN in a bin that carries no data (nothing changes).  Packet 5 has a variance under the floor: its weight hangs on the
    last bits of the packet's mean, whose order of summation the kernel and NumPy do not share, and is held to 1e-13."""
    p = small_params(P=4, carriers=T.MAPS["shuffled"](511) if kind == "shuffled" else None)
    eng = engine_of(p)
    rng = np.random.default_rng(7)
    F, col = 6, p.data_carriers - 1
    idle = np.setdiff1d(np.arange(p.K), col)
    for B in (1, 2, 3, 4):
        vars_ = [rng.chisquare(4, size=(F, 2, p.K)) * 10.0 ** rng.uniform(-3, 1, size=(1, 1, p.K)) for _ in range(B)]
        vars_[B - 1][1, 1, col[17]] = np.nan
        for v in vars_:
            v[2] = 0.0
        vars_[0][3, 0, col[p.C - 3]] = np.inf
        vars_[0][4, 0, idle[0]] = np.nan
        vars_[B - 1][5, :, col[5]] = 1e-12
        w = eng.joint_noise_weights(vars_)
        got, ref = w.cpu().numpy(), JR.weights(vars_, p)
        assert got.dtype == np.float64 and got.shape == ref.shape == (B, F, p.C)
        assert same_bytes(w, eng.joint_noise_weights(vars_))
        assert np.array_equal(got[:, :5], ref[:, :5]) and np.isfinite(got).all()
        assert got[B - 1, 1, 17] == 0.0 and (np.delete(got[:, 1].reshape(-1), (B - 1) * p.C + 17) == 1.0).all()
        assert (got[:, 2] == 1.0).all() and got[0, 3, p.C - 3] == 0.0
        others = np.arange(B * p.C).reshape(B, p.C) != (B - 1) * p.C + 5
        assert np.array_equal(got[:, 5][others], ref[:, 5][others])
        np.testing.assert_allclose(got[B - 1, 5, 5], ref[B - 1, 5, 5], rtol=1e-13)
        assert got[B - 1, 5, 5] < 1e7 / np.mean(JR.carrier_vars(vars_, p)[:, 5])      # (floored: not 1e12)
    with pytest.raises(ValueError, match="joint_noise_weights"):
        eng.joint_noise_weights([])
    with pytest.raises(ValueError, match="joint_noise_weights"):
        eng.joint_noise_weights([np.zeros((2, 2, 511)), np.zeros((3, 2, 511))])
    assert eng.joint_noise_weights([np.zeros((0, 2, 511))] * 2).shape == (2, 0, p.C)


# ---- the weighted detectors ----------------------------------------------------------------------------------------------
def weights_for(p, F, B, seed):
    """Weights over three decades; single branches switched off here and there"""
    rng = np.random.default_rng(seed)
    w = np.exp(1.5 * rng.normal(size=(B, F, p.C)))
    w[rng.random(size=w.shape) < 0.02] = 0.0
    return w


CALLS = dict(mimo=("mimo_detect", JR.detect_mimo, lambda slopes, B: slopes[:B]),
             stbc=("stbc_detect", JR.detect_stbc, lambda slopes, B: slopes[0]))


def check_weighted(code, p, eng, Ys, Hs, slopes, w, packets=None):
    """One weighted call against the restatement (on `packets` alone where given) at the tolerance of the unweighted
    detectors' own comparison, the signs against the restatement's joint argmin, a second call's bytes -> the LLRs"""
    name, restated, _ = CALLS[code]
    call = getattr(eng, name)
    llr = call(Ys, Hs, slopes, weights=w)
    got = llr.cpu().numpy()
    assert got.dtype == np.float32 and same_bytes(llr, call(Ys, Hs, slopes, weights=w))
    part = got
    if packets is not None:
        rows = (np.asarray(packets)[:, None] * p.D + np.arange(p.D)).reshape(-1)
        Ys, Hs, w = [y[rows] for y in Ys], [h[packets] for h in Hs], w[:, packets]
        slopes = [s[packets] for s in slopes] if code == "mimo" else slopes[packets]
        part = got[packets]
    ref, pair = restated(Ys, Hs, slopes, w, p)
    joint_held(part, ref, pair, p.const_bits, clear_share=0.95)
    return got


@pytest.mark.parametrize("kind", ["qpsk", "shuffled"])
@pytest.mark.parametrize("code", ["mimo", "stbc"])
def test_weighted_detect_against_the_restatement(code, kind):
    p = small_params(P=4, D=7 if code == "mimo" else 6, carriers=T.MAPS["shuffled"](511) if kind == "shuffled" else None)
    eng = engine_of(p)
    name, _, pick = CALLS[code]
    Ys, Hs, slopes = detect_inputs(p, F3, 4, len(kind) + len(code))
    for B in (1, 2, 3, 4):
        w = weights_for(p, F3, B, B)
        w[:, 1, 40] = 0.0                                   # every branch off at one carrier of one packet
        w[0, 2, p.C - 2] = np.inf                              # a weight that is not finite: that branch is left out there
        sl = pick(slopes, B)
        got = check_weighted(code, p, eng, Ys[:B], Hs[:B], sl, w)
        dead = got[1, :, :, 40] if code == "mimo" else got[1, :, 40]
        assert not dead.any() and not np.signbit(dead).any()
        # weights all 1.0: the unweighted call, to the same tolerance
        call = getattr(eng, name)
        plain = call(Ys[:B], Hs[:B], sl).cpu().numpy()
        ones = call(Ys[:B], Hs[:B], sl, weights=np.ones((B, F3, p.C))).cpu().numpy()
        np.testing.assert_allclose(ones, plain, rtol=1e-6, atol=1e-9 * np.abs(plain).max())
        # every weight 0: +0 everywhere, no sign bit
        none = call(Ys[:B], Hs[:B], sl, weights=np.zeros((B, F3, p.C))).cpu().numpy()
        assert not none.any() and not np.signbit(none).any()
        for bad in (np.ones((B, F3, p.C - 1)), np.ones((B + 1, F3, p.C))):
            with pytest.raises(ValueError, match=f"{name}: weights"):
                call(Ys[:B], Hs[:B], sl, weights=bad)


@pytest.mark.parametrize("code", ["mimo", "stbc"])
def test_weighted_detect_runs_of_symbols_per_workgroup(code):
    """64 packets of 96 symbols on 257 carriers: a workgroup takes a run of consecutive symbols (or pairs) under the one
    weight it read ahead of the loop; three packets are held to the restatement."""
    p = small_params(P=4, D=96, carriers=np.arange(5, 262))
    eng = engine_of(p)
    Ys, Hs, slopes = detect_inputs(p, 64, 2, 61)
    check_weighted(code, p, eng, Ys, Hs, CALLS[code][2](slopes, 2), weights_for(p, 64, 2, 5), packets=[0, 37, 63])


def test_weighted_detect_abi_refusals():
    import ctypes as C
    from gf3_audio_modem_amd import _lib
    p = small_params(P=4, D=6)
    eng = engine_of(p)
    Ys, Hs, slopes = detect_inputs(p, 2, 2, 8)
    dY, dH = [eng._dev(y) for y in Ys], [eng._dev(h) for h in Hs]
    dS = [eng._dev(s, torch.float64) for s in slopes]
    w = eng._dev(np.ones((2, 2, p.C)), torch.float64)
    out = torch.empty(2 * 2 * p.D * p.C * 2, dtype=torch.float32, device="cuda")
    tab = lambda xs: (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    lib, q = eng.lib, _lib.ptr(out)
    assert lib.gf3_mimo_detect_nw(eng._h, 2, tab(dY), tab(dH), tab(dS), None, 0, q, None) == 0                  # F == 0: a no-op
    assert lib.gf3_mimo_detect_nw(eng._h, 2, tab(dY), tab(dH), tab(dS), None, 2, q, None) == _lib.GF3_EINVAL
    assert b"gf3_mimo_detect_nw" in lib.gf3_last_error(None)
    assert lib.gf3_stbc_detect_nw(eng._h, 2, tab(dY), tab(dH), _lib.ptr(dS[0]), None, 2, q, None) == _lib.GF3_EINVAL
    assert b"gf3_stbc_detect_nw" in lib.gf3_last_error(None)
    assert lib.gf3_mimo_detect_nw(eng._h, 5, tab(dY), tab(dH), tab(dS), _lib.ptr(w), 2, q, None) == _lib.GF3_EINVAL
    assert lib.gf3_joint_noise_weights(eng._h, 0, None, 2, _lib.ptr(w), None) == _lib.GF3_EINVAL
    assert b"gf3_joint_noise_weights" in lib.gf3_last_error(None)
    assert lib.gf3_joint_noise_weights(None, 1, None, 0, None, None) == _lib.GF3_EINVAL
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------------------------------------
def facade(**attrs):
    from gf3_audio_modem_amd.OFDM import receiver
    rx = receiver("A2", encoding="None", no_pilots=4, packet_length=4)
    for k, v in attrs.items():
        setattr(rx, k, v)
    return rx


def oracle_params(rx):
    pts, bt = orc.qpsk_table()
    return orc.RxParams(N=4096, CP=224, P=4, D=4, lo=100, hi=1500, const_points=pts, const_bits=bt,
                        known_bits=np.asarray(rx.known_sequence, dtype=np.uint8))


# The levels come from the restatement alone (no kernel): the comparison below excuses the cells whose restated LLR is as
# good as a tie and caps them at 0.1 %.  With two microphones the restated MIMO chain itself has 26 to 36 such cells of
# 22 400 at 14 dB (three seeds) -- over the cap before any kernel has run -- 15 to 21 at 20 dB and 0 to 6 at 22 dB, where
# it still makes 24 to 27 bit errors unweighted and 3 to 12 weighted; the space-time code has none at 10 dB.
LEVEL_DB = dict(mimo=22.0, stbc=10.0)


@functools.lru_cache(maxsize=None)
def noisy_recordings(code):
    """Two packets of mode A2 (a pair for transmit_mimo) through the scenario's room, the restatement's coloured noise on
    both microphones -> (payload, recordings)"""
    rx = facade()
    payload = np.random.default_rng(3).integers(0, 2, size=2 * 4 * 2800)
    np.random.seed(5)
    tx2 = quiet(rx.transmit_mimo if code == "mimo" else rx.transmit_stbc, payload)
    tx2 = np.concatenate([np.zeros((2, LEAD)), tx2, np.zeros((2, TAIL))], axis=1)
    return payload, JR.coloured(MR.through(tx2), tx2, LEVEL_DB[code], oracle_params(rx))


@pytest.mark.parametrize("code", ["mimo", "stbc"])
def test_receive_under_pilot_measured_weights(code):
    payload, rec = noisy_recordings(code)
    rx = facade(joint_weighting="noise")
    p = oracle_params(rx)
    bits, _, _ = quiet(rx.receive_mimo if code == "mimo" else rx.receive_stbc, rec)
    o = (JR.receive_mimo if code == "mimo" else JR.receive_stbc)(rec, p)
    assert np.array_equal(rx.last_branch_starts, o["starts"])
    # the bits are the restated chain's, but for the cells whose restated LLR is as good as a tie
    tie = np.abs(o["llr_w"]) < 1e-3 * np.median(np.abs(o["llr_w"]))
    differ = bits != o["bits_w"]
    plain = quiet(facade().receive_mimo if code == "mimo" else facade().receive_stbc, rec)[0]
    print(f"{code}: {int(tie.sum())} of {tie.size} cells excused, {int(differ.sum())} bits differ from the restated chain; bit errors "
          f"{int(np.sum(bits != payload))} weighted, {int(np.sum(plain != payload))} unweighted")
    assert bits.shape == o["bits_w"].shape and tie.mean() <= 1e-3 and not differ[~tie].any()
    # what it publishes
    F = 1 if code == "mimo" else 2
    snr, branch = rx.last_snr_db, rx.last_branch_snr_db
    assert snr.dtype == branch.dtype == np.float64 and branch.shape == (2, F, 2, 1400)
    assert snr.shape == ((F, 2, 1400) if code == "mimo" else (F, 1400))
    for got, ref in ((snr, o["snr_db"]), (branch, o["branch_snr_db"])):
        fin = np.isfinite(ref)
        assert fin.mean() > 0.99 and np.array_equal(np.isfinite(got), fin)
        print(f"{code}: worst deviation {np.abs(got[fin] - ref[fin]).max():.2e} dB, median {np.median(ref[fin]):.1f} dB")
        np.testing.assert_allclose(got[fin], ref[fin], rtol=0, atol=1e-6)
    # the noisy bands show: microphone 0 is worse below bin 150, microphone 1 above bin 250 (data carriers 100 .. 1499)
    lowband, highband = slice(0, 50), slice(150, 412)
    assert np.median(branch[0][..., lowband]) < np.median(branch[0][..., highband]) - 6.0
    assert np.median(branch[1][..., highband]) < np.median(branch[1][..., lowband]) - 6.0
    # under "csi" both stay None
    assert facade().last_snr_db is None
    csi = facade()
    quiet(csi.receive_mimo if code == "mimo" else csi.receive_stbc, rec)
    assert csi.last_snr_db is None and csi.last_branch_snr_db is None
