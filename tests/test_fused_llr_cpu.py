"""The fused sample-to-LLR path (gf3_demod_frames_llr, Engine.demod_frames_llr, CamG.fused_llr): what can be checked
without a GPU -- the binding, and the argument rules of receive() that apply before any GPU work."""
import ctypes as C

import numpy as np
import pytest

from gf3_audio_modem_amd import _lib
from gf3_audio_modem_amd.OFDM import receiver


def test_the_call_is_bound_with_its_argument_types():
    assert "gf3_demod_frames_llr" in _lib.exported_names()
    res, args = _lib._SIGS["gf3_demod_frames_llr"]
    assert res is C.c_int
    # ctx, in, n_in, offsets, F, llr, weight, Hs, He, slope, status, work, mode, stream
    assert args == [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]


def test_fused_llr_is_off_by_default():
    assert receiver("A2", encoding="QCLDPC-1/2").fused_llr is False


@pytest.mark.parametrize("weighting", ["noise", "noise2d"])
def test_fused_llr_refuses_the_noise_weights_before_any_gpu_work(weighting, capsys):
    rx = receiver("A2", encoding="QCLDPC-1/2")
    rx.fused_llr = True
    rx.llr_weighting = weighting
    with pytest.raises(ValueError, match="fused_llr"):
        rx.receive(np.zeros(1000))
    capsys.readouterr()


def _outcome(rx, sig):
    try:
        out = rx.receive(sig)
    except Exception as e:                                # noqa: BLE001  (the outcome itself is what is compared)
        return type(e), str(e)
    return tuple(np.asarray(v).tobytes() for v in out)


def test_fused_llr_is_ignored_by_the_hard_decision_encodings(capsys):
    """With "XOR" the attribute changes nothing: receive() ends as it does without it (for want of a GPU where there is
    none), even with a weighting the fused path would refuse."""
    sig = np.zeros(20000)
    plain = receiver("A2", encoding="XOR")
    fused = receiver("A2", encoding="XOR")
    fused.fused_llr = True
    fused.llr_weighting = "noise"
    assert _outcome(plain, sig) == _outcome(fused, sig)
    capsys.readouterr()
