"""receive() and receive_diversity() end to end, option by option, against what the commit before the receive plan gave on
the MI355X: SHA-256 digests of the transmitted signal, the three returned arrays, `no_packets`, `_last_slope` and every
`last_*` attribute, and the number of bit errors against the message (tests/golden/receive_pipeline.json; None is recorded
as null, `last_decode_report` by its values, short integer arrays as lists).
The parent was recorded twice, in two processes, and every item came out the same in both: all of them are held exactly.

    PYTHONPATH=TREE python tests/test_receive_pipeline_gpu.py --record OUT.json      (TREE: a built checkout to record)
    python tests/test_receive_pipeline_gpu.py --merge A.json B.json tests/golden/receive_pipeline.json

Geometry: mode "A2" with no_pilots = 2 and packet_length = 4, three packets from a transmitter with the case's settings
under np.random.seed, 300 samples of lead and 400 of tail, white noise from a seeded default_rng on the host at the case's
SNR (noise power against the signal's mean power; 10 to 22 dB, chosen per case from a sweep on the parent so that the
uncoded cases have some hundred bit errors and the coded ones some failed codewords: with two pilot symbols per side the
phase-slope fit, and with it every decision, falls apart below about 12 dB); the blanking case plants one click of 40 samples at 30 times the
signal's RMS in the first packet; a second recording of the diversity cases is delayed by 5 samples and has its own noise.
The feedback case's SNR is one at which the parent reports feedback_passes >= 1, the blanking case reports blanked
samples: the recorder asserts both."""
import contextlib
import hashlib
import io
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "receive_pipeline.json")
K_HALF = 768                                                    # message bits of a rate-1/2 codeword of 1536
LOADING = "the 6/4/2/0 table"
QC = "QCLDPC-1/2"
# name: (call, recordings, encoding, settings, SNR in dB, click)
CASES = {
    "none": ("receive", 1, "None", {}, 18.0, False),
    "xor": ("receive", 1, "XOR", {}, 18.0, False),
    "qc_csi": ("receive", 1, QC, {}, 14.0, False),
    "qc_csi_fused": ("receive", 1, QC, {"fused_llr": True}, 14.0, False),
    "qc_noise_il_crc_outer": ("receive", 1, QC, {"llr_weighting": "noise", "interleave": True, "codeword_crc": True,
                                                 "outer_code": (4, 2)}, 14.0, False),
    "qc_noise2d_il": ("receive", 1, QC, {"llr_weighting": "noise2d", "interleave": True}, 14.0, False),
    "qc_track_feedback_crc": ("receive", 1, QC, {"phase_tracking": True, "decoder_feedback": 1, "codeword_crc": True}, 13.0, False),
    "qc_blank_clock_denoise_noise": ("receive", 1, QC, {"impulse_blanking": True, "clock_correction": 100.0,
                                                        "channel_denoising": True, "llr_weighting": "noise"}, 14.0, True),
    "xor_clock_auto": ("receive", 1, "XOR", {"clock_correction": "auto"}, 18.0, False),
    "qc_loading_noise_denoise": ("receive", 1, QC, {"bit_loading": LOADING, "llr_weighting": "noise",
                                                    "channel_denoising": True}, 22.0, False),
    "none_loading": ("receive", 1, "None", {"bit_loading": LOADING}, 22.0, False),
    "xor_chunked": ("receive", 1, "XOR", {"host_chunk_samples": 1 << 16}, 18.0, False),
    "div1_none": ("receive_diversity", 1, "None", {}, 18.0, False),
    "div2_xor": ("receive_diversity", 2, "XOR", {}, 12.0, False),
    "div2_qc_noise_il_clock_denoise": ("receive_diversity", 2, QC, {"llr_weighting": "noise", "interleave": True,
                                                                    "clock_correction": "auto", "channel_denoising": True}, 10.0, False),
}


def a2_order():
    order = np.zeros(1400, dtype=np.uint8)
    order[:500], order[500:900], order[900:1300] = 6, 4, 2
    return order


def configured(cls, encoding, settings):
    obj = cls("A2", encoding=encoding, no_pilots=2, packet_length=4)
    for name, value in settings.items():
        setattr(obj, name, a2_order() if value is LOADING else value)
    return obj


def signals(name):
    """The transmit side of one case, on a fresh transmitter -> (message, transmitted signal, the B noisy recordings)."""
    from gf3_audio_modem_amd import OFDM
    _, B, encoding, settings, snr_db, click = CASES[name]
    seed = 1000 + list(CASES).index(name)
    np.random.seed(seed)
    tx = configured(OFDM.transmitter, encoding, {k: v for k, v in settings.items() if k != "host_chunk_samples"})
    cap, NG = tx.outer_layout(3)
    if encoding == QC:
        words = NG * tx.outer_code[0] if tx.outer_code else cap
        n_msg = words * (K_HALF - 32 * bool(tx.codeword_crc))
    else:
        n_msg = 3 * tx.packet_length * tx.loaded_bits_per_symbol
    message = np.random.default_rng(seed).integers(0, 2, size=n_msg)
    with contextlib.redirect_stdout(io.StringIO()):
        sent = tx.transmit(message)
    assert tx.no_packets == 3
    rms = float(np.sqrt(np.mean(sent ** 2)))
    clean = np.concatenate([np.zeros(300), sent, np.zeros(400)])
    if click:
        at = 300 + tx.chirp_length + 3 * (tx.ofdm_symbol_size + tx.cp_length) + 1000
        clean[at: at + 40] += 30.0 * rms * np.random.default_rng(seed + 9).choice([-1.0, 1.0], size=40)
    recordings = []
    for b in range(B):
        r = np.concatenate([np.zeros(5 * b), clean])
        recordings.append(r + rms * 10.0 ** (-snr_db / 20.0) * np.random.default_rng(seed + 1 + b).standard_normal(len(r)))
    return message, sent, recordings


def run(name):
    """One case on a fresh receiver -> {item: value}."""
    from gf3_audio_modem_amd import OFDM
    call, _, encoding, settings, _, _ = CASES[name]
    message, sent, recordings = signals(name)
    rx = configured(OFDM.receiver, encoding, settings)
    with contextlib.redirect_stdout(io.StringIO()):
        bits, Hs, He = rx.receive(recordings[0]) if call == "receive" else rx.receive_diversity(recordings)
    items = {"sent": sent, "bits": bits, "Hs": Hs, "He": He, "no_packets": rx.no_packets, "_last_slope": rx._last_slope,
             "bit_errors": int(np.sum(np.asarray(bits[:len(message)]) != message))}
    items.update({k: v for k, v in sorted(vars(rx).items()) if k.startswith("last_")})
    return items


def recorded(value):
    """What the file holds of one item: None, a number, a short integer array as a list, any other array as its digest."""
    if value is None or isinstance(value, (bool, int, float, str)):
        return value
    if isinstance(value, dict):
        return {k: recorded(v) for k, v in value.items()}
    if isinstance(value, np.generic):
        return value.item()
    a = np.ascontiguousarray(value)
    if a.dtype.kind in "iu" and a.size <= 64:
        return a.reshape(-1).tolist()
    return {"dtype": str(a.dtype), "shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


@pytest.mark.parametrize("name", list(CASES))
def test_case_gives_what_the_parent_gave(name):
    want = json.load(open(GOLD))[name]
    got = {k: recorded(v) for k, v in run(name).items()}
    print(f"{name}: bit errors {got['bit_errors']}, report {got.get('last_decode_report')}")
    assert sorted(got) == sorted(want)
    assert [k for k in want if got[k] != want[k]] == []


def main(argv):
    if argv[0] == "--record":
        out = {}
        for name in CASES:
            out[name] = {k: recorded(v) for k, v in run(name).items()}
            print(f"{name}: bit errors {out[name]['bit_errors']}, report {out[name].get('last_decode_report')}", flush=True)
        assert out["qc_track_feedback_crc"]["last_decode_report"]["feedback_passes"] >= 1
        assert run("qc_blank_clock_denoise_noise")["last_blanked"].sum() > 0
        json.dump(out, open(argv[1], "w"), indent=0, sort_keys=True)
    elif argv[0] == "--merge":
        a, b = json.load(open(argv[1])), json.load(open(argv[2]))
        differ = [(c, k) for c in a for k in a[c] if a[c][k] != b[c][k]]
        print("items that differ between the two recordings:", differ)
        assert not differ, "not reproducible on the recorded tree itself: such an item needs a measured tolerance, not a digest"
        with open(argv[3], "w") as fh:
            json.dump(a, fh, indent=0, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
