"""The self-normalised chirp detection without a GPU: the rule itself (tests/detect_ref.py) on the project's real recording,
the segmentation state machine of the live receiver on hand-written detections, and the refusals of the facade."""
import contextlib
import io

import numpy as np
import pytest

from oracle import gf3_oracle as orc
from tests import detect_ref
from tests.util import load, modeA2_params

TAU = 0.3


@pytest.fixture(scope="module")
def rec():
    g = load("g6_realrec")
    p = modeA2_params(g["known_bits"])
    r = g["wav_u8"] / 1.0
    return dict(r=r, p=p, chirp=orc.chirp_replica(p), peaks=g["peaks"].astype(np.int64), rho=detect_ref.rho(r, orc.chirp_replica(p))[0])


def test_real_recording_detections_and_margin(rec):
    r, p, peaks, q = rec["r"], rec["p"], rec["peaks"], rec["rho"]
    assert np.array_equal(detect_ref.detect(q, len(r), p.Lc, TAU), peaks)
    at = q[peaks + 1]
    print("rho at the chirps:", at)
    assert np.all(at > 0.5) and np.all(at <= 1.0)
    g = np.arange(len(q))
    far = (g >= p.Lc - 1) & (g <= len(r) - 1) & np.all(np.abs(g[:, None] - (peaks + 1)[None, :]) > p.Lc, axis=1)
    print("largest rho away from the chirps:", q[far].max())
    assert q[far].max() < TAU
    assert np.all(np.abs(q) <= 1.0 + 1e-9)


def test_level_varying_recording_keeps_every_chirp(rec):
    """The second packet's stretch at a fifth of the level: the reference's rule loses that packet, this one does not."""
    r, p, peaks = rec["r"], rec["p"], rec["peaks"]
    x = r - r.mean()
    x[peaks[1] - p.Lc - 2000: peaks[2] - p.Lc - 2000] *= 0.2
    assert np.array_equal(np.flatnonzero(orc.chirp_method(x, p)), np.delete(peaks, 1))
    q = detect_ref.rho(x, rec["chirp"])[0]
    assert np.array_equal(detect_ref.detect(q, len(x), p.Lc, TAU), peaks)
    # away from the level steps the coefficient is the one of the unscaled recording
    assert np.abs(q[peaks + 1] - rec["rho"][peaks + 1]).max() < 1e-9


def test_rho_does_not_change_under_gain_and_offset(rec):
    r = rec["r"][:400000]
    a, _ = detect_ref.rho(r, rec["chirp"])
    b, _ = detect_ref.rho(3.7 * r - 11.0, rec["chirp"])
    assert np.abs(a - b).max() <= 1e-9


# ---- the segmentation state machine ---------------------------------------------------------------------------------
FRAME, GAP, SLACK = 1000, 300, 50


def drive(detections, steps):
    """Push `detections` in `steps` groups, the horizon following the last one pushed; then the end of the stream."""
    from gf3_audio_modem_amd.live import END, Segmenter
    seg = Segmenter(FRAME, GAP, SLACK)
    closed = []
    for part in np.array_split(np.asarray(detections, dtype=np.int64), steps):
        closed += seg.push(part.tolist(), (int(part[-1]) + 1) if len(part) else 0)
    closed += seg.push([], END)
    assert seg.open == []
    return closed


def test_segmenter_two_transmissions_and_a_lone_chirp():
    a = [100, 1100, 2100, 3100]                              # three packets and the terminating chirp
    b = [9000, 10010, 11005]
    lone = [20000]
    want = [a, b, lone]
    assert drive(a + b + lone, 1) == want
    assert [list(t) for t in detect_ref.segment(a + b + lone, FRAME, GAP, SLACK)] == want
    # one at a time and all at once close the same transmissions
    assert drive(a + b + lone, len(a + b + lone)) == want


def test_segmenter_gap_boundaries():
    from gf3_audio_modem_amd.live import Segmenter
    assert drive([0, FRAME + GAP], 1) == [[0, FRAME + GAP]]                   # exactly frame_len + max_gap: one transmission
    assert drive([0, FRAME + GAP + 1], 2) == [[0], [FRAME + GAP + 1]]         # one more: two lone chirps
    assert drive([0, FRAME - SLACK], 1) == [[0, FRAME - SLACK]]
    assert drive([0, FRAME - SLACK - 1], 2) == [[0], [FRAME - SLACK - 1]]     # a chirp that comes too soon opens the next one
    # the horizon closes a transmission exactly when no detection can extend it any more
    seg = Segmenter(FRAME, GAP, SLACK)
    assert seg.push([0, FRAME], FRAME + 1) == []
    assert seg.push([], 2 * FRAME + GAP) == [] and seg.open == [0, FRAME]
    assert seg.push([], 2 * FRAME + GAP + 1) == [[0, FRAME]] and seg.open == []
    assert seg.force() == []


# ---- refusals of the facade (no GPU: the engine is never reached) -----------------------------------------------------
class Reached(Exception):
    pass


def receive_with(**attrs):
    from gf3_audio_modem_amd.OFDM import receiver

    def reached(*a, **kw):
        raise Reached()
    rx = receiver("A2", encoding="XOR", no_pilots=2, packet_length=4)
    rx._engine = reached
    for k, v in attrs.items():
        setattr(rx, k, v)
    with contextlib.redirect_stdout(io.StringIO()):
        rx.receive(np.zeros(5000))


def test_facade_refusals():
    from gf3_audio_modem_amd import Engine, LiveReceiver
    from gf3_audio_modem_amd.OFDM import receiver
    assert receiver("A2").sync_rule == "global" and receiver("A2").detect_threshold == 0.3 and receiver("A2").sync_report is None
    with pytest.raises(Reached):
        receive_with(sync_rule="local")
    for rule in ("Local", "", None, 1):
        with pytest.raises(ValueError, match="sync_rule must be 'global' or 'local'"):
            receive_with(sync_rule=rule)
    for tau in (0.0, 1.0, -0.2, float("nan"), float("inf"), "0.3", None, True):
        with pytest.raises(ValueError, match="detection threshold"):
            receive_with(sync_rule="local", detect_threshold=tau)
        with pytest.raises(ValueError, match="detection threshold"):
            Engine.check_detect(tau)
    assert Engine.check_detect(0.25) == 0.25
    with pytest.raises(NotImplementedError, match="sync_rule 'local'"):
        receive_with(sync_rule="local", host_chunk_samples=1 << 20)
    # the live receiver refuses at construction what receive() under the local rule refuses
    rx = receiver("A2", no_pilots=2, packet_length=4)
    rx.host_chunk_samples = 1 << 20
    with pytest.raises(NotImplementedError, match="sync_rule 'local'"):
        LiveReceiver(rx)
    rx.host_chunk_samples = None
    rx.detect_threshold = 2.0
    with pytest.raises(ValueError, match="detection threshold"):
        LiveReceiver(rx)
    assert rx.sync_rule == "global"                          # (left as it was)
