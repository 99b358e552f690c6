"""What every option combination of receive(), receive_diversity() and encode() does before the GPU is touched: refuse
(with which exception and which message), reach the engine, or return.  A characterisation: the outcomes are recorded from
the commit before the receive plan (tests/golden/receive_refusals.json) and every later tree must give the same ones.
Which refusal wins when two options conflict is thereby pinned.

    PYTHONPATH=TREE python tests/test_receive_refusals_cpu.py --record FILE      (TREE: a checkout of the tree to record)

The engine is a stand-in whose every attribute access raises `Reached`, and so does the code lookup: a case ends at its
first refusal, at the first use of the GPU ("reached"), or with the call's return ("returned").  decode() is left out: it
goes to torch.cuda directly and answers differently with and without a GPU."""
import contextlib
import io
import itertools
import json
import os
import sys

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "receive_refusals.json")
ENCODINGS = ["None", "XOR", "QCLDPC-1/2"]
CALLS = ["receive", "receive_diversity", "encode"]
LOADING = "the 6/4/2/0 table"                                   # (stands for the array in the lists below and in the file)
DEVIATIONS = [{"llr_weighting": "noise"}, {"llr_weighting": "noise2d"}, {"llr_weighting": "bogus"}, {"interleave": True},
              {"fused_llr": True}, {"phase_tracking": True}, {"decoder_feedback": 1}, {"codeword_crc": True},
              {"outer_code": [4, 2]}, {"bit_loading": LOADING}, {"impulse_blanking": True}, {"clock_correction": "auto"},
              {"channel_denoising": True}, {"graph_output": True}, {"host_chunk_samples": 1 << 20}]
BAD = [{"clock_taps": 48}, {"clock_correction": 5000.0}, {"impulse_blanking": True, "blanking_threshold": -1.0},
       {"impulse_blanking": True, "blanking_guard": -3}, {"channel_denoising": True, "denoise_threshold": 0.0},
       {"channel_denoising": True, "no_pilots": 1}, {"decoder_feedback": -1},
       {"decoder_feedback": 1, "feedback_window": [99, 99]}, {"outer_code": [4]}]
KINDS = ("reached", "returned", "ValueError: ", "NotImplementedError: ")


class Reached(Exception):
    pass


class StandIn:
    def __getattr__(self, name):
        raise Reached(name)


def settings():
    """The deviation sets in enumeration order: every subset of at most three deviations that holds no attribute twice,
    then every bad value alone and after each single deviation (the bad value is applied last)."""
    out = []
    for n in range(4):
        for combo in itertools.combinations(DEVIATIONS, n):
            names = [k for d in combo for k in d]
            if len(set(names)) == len(names):
                out.append([dict(d) for d in combo])
    for bad in BAD:
        out.append([dict(bad)])
        out.extend([dict(d), dict(bad)] for d in DEVIATIONS)
    return out


def a2_order():
    order = np.zeros(1400, dtype=np.uint8)
    order[:500], order[500:900], order[900:1300] = 6, 4, 2
    return order


def outcome(OFDM, encoding, call, deviations):
    rx = OFDM.receiver("A2", encoding=encoding, no_pilots=2, packet_length=4)
    rx._engine = lambda *a, **kw: StandIn()
    graph_output = False
    for dev in deviations:
        for name, value in dev.items():
            if name == "graph_output":
                graph_output = value
            else:
                value = a2_order() if value == LOADING else tuple(value) if isinstance(value, list) else value
                setattr(rx, name, value)
    z = np.zeros(5000)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            if call == "receive":
                rx.receive(z, graph_output=graph_output)
            elif call == "receive_diversity":
                rx.receive_diversity([z, z], graph_output=graph_output)
            else:
                rx.encode(np.zeros(10, int))
    except Reached:
        return "reached"
    except Exception as e:
        return f"{type(e).__name__}: {e}"
    return "returned"


def outcomes():
    from gf3_audio_modem_amd import OFDM

    def no_code(*a, **kw):
        raise Reached("_qcldpc_code")
    kept, OFDM._qcldpc_code = OFDM._qcldpc_code, no_code
    state = np.random.get_state()                               # (encode() draws its fill from the global generator)
    try:
        return [outcome(OFDM, enc, call, devs) for enc in ENCODINGS for call in CALLS for devs in settings()]
    finally:
        OFDM._qcldpc_code = kept
        np.random.set_state(state)


def test_every_combination_does_what_it_did():
    want = json.load(open(GOLD))
    assert want["encodings"] == ENCODINGS and want["calls"] == CALLS
    assert want["deviations"] == DEVIATIONS and want["bad_values"] == BAD          # a changed enumeration fails here
    assert all(s.startswith(KINDS) for s in want["outcomes"])
    got = outcomes()
    assert len(got) == len(want["index"]) == len(ENCODINGS) * len(CALLS) * len(settings())
    cases = [(enc, call, devs) for enc in ENCODINGS for call in CALLS for devs in settings()]
    wrong = [(c, g, want["outcomes"][i]) for c, g, i in zip(cases, got, want["index"]) if g != want["outcomes"][i]]
    for case, g, w in wrong[:20]:
        print(f"{case}:\n   now      {g}\n   recorded {w}")
    assert not wrong, f"{len(wrong)} of {len(got)} cases changed"
    assert os.path.getsize(GOLD) < 256 * 1024


if __name__ == "__main__":
    assert sys.argv[1] == "--record"
    got = outcomes()
    distinct = sorted(set(got))
    with open(sys.argv[2], "w") as fh:
        json.dump({"encodings": ENCODINGS, "calls": CALLS, "deviations": DEVIATIONS, "bad_values": BAD, "outcomes": distinct,
                   "index": [distinct.index(g) for g in got]}, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{len(got)} cases, {len(distinct)} distinct outcomes")
