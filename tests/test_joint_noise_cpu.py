"""The two-speaker receive paths under coloured noise, without a GPU: the interface is declared, the façade refuses what it
must, and the NumPy restatement (tests/joint_noise_ref.py) shows what the feature is for -- pilot-measured weights in the
joint metric against the unweighted metric, in noise that is 6 x louder in one band per microphone and in white noise --
and that the estimate measures what it says (nothing on a noiseless recording, N sigma^2 in white noise).
tests/test_joint_noise_gpu.py holds the kernels to the same restatement.

Scenario: `small_params` of tests/test_mimo_cpu.py with P = 4, D = 6 (N = 1024, CP = 64, data bins 5 .. 399), bits of seed
3, mimo_ref.through's room, lead 300, tail 400, window advance 16; MIMO at 14 dB from both microphones, the space-time code
at 10 dB from both."""
import functools
import os
import re

import numpy as np
import pytest

from tests import joint_noise_ref as JR
from tests import mimo_ref as MR
from tests import stbc_ref as SR
from tests.test_mimo_cpu import small_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gf3_mimo_pilot_noise", "gf3_joint_noise_weights", "gf3_mimo_detect_nw", "gf3_stbc_detect_nw")
ADVANCE = 16


def test_interface_is_declared():
    from gf3_audio_modem_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "gf3rx.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), name
        assert name in _lib.exported_names(), name
    # the weighted calls are the unweighted ones with one more pointer; those keep their signatures
    for name in ("gf3_mimo_detect", "gf3_stbc_detect"):
        res, args = _lib._SIGS[name]
        assert len(args) == 8
        assert _lib._SIGS[name + "_nw"] == (res, args[:5] + [args[4]] + args[5:])
    assert "gf3rx_joint_noise" in build.UNITS and os.path.exists(os.path.join(build.CSRC, "gf3rx_joint_noise.hip"))


def test_facade_refuses_without_gpu():
    from gf3_audio_modem_amd.OFDM import receiver
    x = np.zeros(1000)

    def rx(**attrs):
        r = receiver("A2", encoding="None", no_pilots=attrs.pop("no_pilots", 4), packet_length=4)
        for k, v in attrs.items():
            setattr(r, k, v)
        return r
    assert rx().joint_weighting == "csi" and rx().last_snr_db is None and rx().last_branch_snr_db is None
    for call in ("receive_mimo", "receive_stbc"):
        for value in ("flat", "noise2d", "", None, 1, True):
            with pytest.raises(ValueError, match="joint_weighting"):
                getattr(rx(joint_weighting=value), call)([x, x])
        with pytest.raises(ValueError, match="joint_weighting.*no_pilots"):
            getattr(rx(joint_weighting="noise", no_pilots=2), call)([x, x])
        # llr_weighting keeps its meaning and its refusal here, whatever joint_weighting says
        for joint in ("csi", "noise"):
            with pytest.raises(ValueError, match="llr_weighting"):
                getattr(rx(llr_weighting="noise", joint_weighting=joint), call)([x, x])
        # the cover's own refusal still comes first
        with pytest.raises(ValueError, match="no_pilots must be even"):
            getattr(rx(joint_weighting="noise", no_pilots=3), call)([x, x])


# ---- the scenario --------------------------------------------------------------------------------------------------------
FILL = (1 + 1j) / np.sqrt(2)


@functools.lru_cache(maxsize=None)
def scenario(code):
    """-> (p, bits, the speakers' streams, the noiseless recordings [microphone 0, microphone 1])"""
    p = small_params(P=4, D=6)
    packets = 4 if code == "mimo" else 2
    bits = np.random.default_rng(3).integers(0, 2, size=packets * p.D * p.C * p.mu)
    tx = MR.tx_mimo if code == "mimo" else SR.tx_stbc
    tx2 = tx(bits, np.full(p.K - p.C, FILL), p, lead=300, tail=400)
    return p, bits, tx2, MR.through(tx2)


RECEIVE = dict(mimo=JR.receive_mimo, stbc=JR.receive_stbc)
LEVEL_DB = dict(mimo=14.0, stbc=10.0)


@functools.lru_cache(maxsize=None)
def errors(code, boost):
    """Hard bit errors of the restated chains in the scenario's noise -> (unweighted, weighted, number of bits)"""
    p, bits, tx2, clean = scenario(code)
    o = RECEIVE[code](JR.coloured(clean, tx2, LEVEL_DB[code], p, boost=boost), p, advance=ADVANCE)
    plain, weighted = int(np.sum(o["bits"] != bits)), int(np.sum(o["bits_w"] != bits))
    print(f"{code}, {LEVEL_DB[code]} dB, boost {boost}: {plain} bit errors unweighted, {weighted} weighted, of {len(bits)}")
    return plain, weighted, len(bits)


@pytest.mark.parametrize("code", ["mimo", "stbc"])
def test_weights_pay_under_coloured_noise(code):
    """6 x the noise amplitude in bins [0, 150) at microphone 0 and [250, 512) at microphone 1: the weighted metric leaves at
    most a quarter of the unweighted metric's bit errors.  (Measured with this restatement: MIMO 123 against 1066 of
    18 960, the space-time code 5 against 384 of 9 480: the cap leaves a factor of two and more.)"""
    plain, weighted, n = errors(code, JR.BOOST)
    assert plain > 0 and 4 * weighted <= plain


@pytest.mark.parametrize("code", ["mimo", "stbc"])
def test_weights_cost_nothing_in_white_noise(code):
    """The same levels without the boost: the estimate's own scatter (two degrees of freedom per block and carrier at P = 4)
    may cost at most 0.1 % of the bits.  (Measured: MIMO 31 against 27, the space-time code 0 against 0.)"""
    plain, weighted, n = errors(code, 1.0)
    assert weighted <= plain + 1e-3 * n


# ---- the estimate ----------------------------------------------------------------------------------------------------------
def estimates(r, p):
    from oracle import gf3_oracle as orc
    st = orc.frame_starts(orc.chirp_method(r, p)) - ADVANCE
    H, status = MR.pilots(r, st, p)
    assert not status.any()
    return st, H


@pytest.mark.parametrize("code", ["mimo", "stbc"])
def test_estimate_of_a_noiseless_recording_is_rounding(code):
    p, bits, tx2, clean = scenario(code)
    for r in clean:
        st, H = estimates(r, p)
        v, status = JR.pilot_noise(r, st, H, p)
        assert v.shape == (len(st), 2, p.K) and v.dtype == np.float64 and status.tolist() == [0] * len(st)
        power = (np.abs(H) ** 2).sum(axis=2)                    # |H0|^2 + |H1|^2 per packet, side and carrier
        print(f"{code}: largest v / |H|^2 on a noiseless recording {np.max(v / power):.1e}")
        assert (v < 1e-20 * power).all()
    # a packet cut at either end: status 1 and NaN rows, the neighbour untouched
    r = clean[0]
    st, H = estimates(r, p)
    cut = np.array([-1, st[0], len(r) - p.M * p.S + 1])
    Hc = np.stack([np.full_like(H[0], np.nan), H[0], np.full_like(H[0], np.nan)])
    vc, sc = JR.pilot_noise(r, cut, Hc, p)
    assert sc.tolist() == [1, 0, 1] and np.isnan(vc[[0, 2]]).all() and np.array_equal(vc[1], JR.pilot_noise(r, st, H, p)[0][0])
    with pytest.raises(ValueError, match="P >= 4"):
        JR.pilot_noise(r, st, H[:, :, :, :], small_params(P=2, D=6))


def test_estimate_in_white_noise_is_n_sigma_squared():
    """White noise of deviation sigma per sample: the unnormalised N-point transform of mimo_ref.pilots carries it to
    N sigma^2 per bin, the known symbols have unit magnitude, and 1 / (P - 2) makes the residual's mean square unbiased.  The
    mean over carriers, sides and packets (about 4000 estimates of two complex degrees of freedom each) is held to 10 %."""
    p, bits, tx2, clean = scenario("mimo")
    assert np.allclose(np.abs(p.known_symbols()), 1.0)
    sigma = 0.05 * SR.body_rms(tx2)
    for b, r in enumerate(clean):
        noisy = r + sigma * np.random.default_rng(40 + b).normal(size=len(r))
        st, H = estimates(noisy, p)
        v, _ = JR.pilot_noise(noisy, st, H, p)
        ratio = v.mean() / (p.N * sigma ** 2)
        print(f"microphone {b}: mean v / (N sigma^2) = {ratio:.3f}")
        assert abs(ratio - 1.0) < 0.1
        # and the weights are its reciprocal on the data carriers, to the same 10 % on average
        w = JR.weights([v], p)
        assert w.shape == (1, len(st), p.C) and abs(np.mean(1.0 / w) / (p.N * sigma ** 2) - 1.0) < 0.1
