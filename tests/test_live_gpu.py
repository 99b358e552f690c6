"""LiveReceiver through the facade: a stream of 0.3 s of weak noise, transmission A (3 packets), 0.5 s of silence,
transmission B (2 packets at 0.05 x), a lone chirp -- fed in blocks, the transmissions decoded as they end."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QC = "QCLDPC-1/2"
CASES = {"xor": ("XOR", {}), "qc_crc": (QC, {"codeword_crc": True})}
LEAD, SILENCE, PAUSE, TAIL = 14400, 24000, 1000, 100


def configured(cls, encoding, settings):
    obj = cls("A2", encoding=encoding, no_pilots=2, packet_length=4)
    for name, value in settings.items():
        setattr(obj, name, value)
    return obj


def quiet(f, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **kw)


_made = {}


def scene(name):
    """-> dict(stream, messages [A, B], spans [(first sample, one past the last) of A and of B])."""
    if name in _made:
        return _made[name]
    from gf3_audio_modem_amd import OFDM
    encoding, settings = CASES[name]
    np.random.seed(31)
    rng = np.random.default_rng(32)
    tx = configured(OFDM.transmitter, encoding, settings)
    messages, sent = [], []
    for F in (3, 2):
        cap, _ = tx.outer_layout(F)
        n_msg = cap * (768 - 32) if encoding == QC else F * tx.packet_length * tx.data_bits_per_symbol
        messages.append(rng.integers(0, 2, size=n_msg))
        sent.append(np.asarray(quiet(tx.transmit, messages[-1]), dtype=np.float64))
        assert tx.no_packets == F
    chirp = tx.sync_chirp()
    parts = [1e-3 * rng.standard_normal(LEAD), sent[0], np.zeros(SILENCE), 0.05 * sent[1], np.zeros(PAUSE), 0.05 * chirp, np.zeros(TAIL)]
    a0 = LEAD
    b0 = LEAD + len(sent[0]) + SILENCE
    _made[name] = dict(stream=np.concatenate(parts), messages=messages, spans=[(a0, a0 + len(sent[0])), (b0, b0 + len(sent[1]))],
                       Lc=len(chirp))
    return _made[name]


def listen(name, blocks):
    from gf3_audio_modem_amd import LiveReceiver, OFDM
    sc = scene(name)
    rx = configured(OFDM.receiver, *CASES[name])
    live = LiveReceiver(rx)
    got, at = [], 0
    for size in blocks:
        got += live.feed(sc["stream"][at: at + size])
        at += size
        if at >= len(sc["stream"]):
            break
    assert at >= len(sc["stream"])
    got += live.flush()
    assert rx.sync_rule == "global"
    return got, live.events


def test_live_receiver_survives_a_cut_and_an_endless_transmission():
    """What a listener must survive becomes an event: a stream that ends inside transmission A's third packet, and a
    transmission that outgrows max_transmission_samples."""
    from gf3_audio_modem_amd import LiveReceiver, OFDM
    sc = scene("xor")
    (lo, hi), Lc, msg = sc["spans"][0], sc["Lc"], sc["messages"][0]
    per_packet = len(msg) // 3
    frame = (hi - lo - Lc) // 3
    # the end of the stream 30 000 samples into the third packet's body: two packets decoded, the third reported as cut off
    live = LiveReceiver(configured(OFDM.receiver, *CASES["xor"]))
    got = []
    for at in range(0, lo + 2 * frame + Lc + 30000, 9600):
        got += live.feed(sc["stream"][at: min(at + 9600, lo + 2 * frame + Lc + 30000)])
    assert got == []
    got = live.flush()
    assert [e["kind"] for e in live.events] == ["cut_packet"] and live.events[0]["start_sample"] == lo + 2 * frame + Lc
    assert len(got) == 1 and got[0].no_packets == 2 and np.array_equal(got[0].bits, msg[: 2 * per_packet])
    # a transmission longer than the limit is closed where it stands; listening goes on with the chirps that follow
    live = LiveReceiver(configured(OFDM.receiver, *CASES["xor"]), max_transmission_samples=100000)
    got = []
    for at in range(0, hi + 20000, 9600):
        got += live.feed(sc["stream"][at: min(at + 9600, hi + 20000)])
    got += live.flush()
    assert [e["kind"] for e in live.events] == ["forced_close"] and live.events[0]["start_sample"] == lo + Lc
    assert [t.no_packets for t in got] == [1, 1] and [t.start_sample for t in got] == [lo + Lc, lo + 2 * frame + Lc]
    assert np.array_equal(got[0].bits, msg[:per_packet]) and np.array_equal(got[1].bits, msg[2 * per_packet:])


@pytest.mark.parametrize("name", list(CASES))
def test_live_receiver_decodes_transmissions_as_they_end(name):
    from gf3_audio_modem_amd import OFDM
    sc = scene(name)
    n, Lc = len(sc["stream"]), sc["Lc"]
    even, ev_even = listen(name, [4800] * (n // 4800 + 1))
    sizes = np.random.default_rng(5).integers(1, 20000, size=n // 2000).tolist()
    odd, ev_odd = listen(name, sizes)
    for got, events in ((even, ev_even), (odd, ev_odd)):
        assert [t.no_packets for t in got] == [3, 2]
        assert [e["kind"] for e in events] == ["lone_chirp"]
        for t, msg, (lo, hi) in zip(got, sc["messages"], sc["spans"]):
            assert t.start_sample == lo + Lc and np.array_equal(t.bits[: len(msg)], msg)
            assert len(t.rho) == t.no_packets + 1 and min(t.rho) > 0.9
            assert (t.decode_report is None) == (name == "xor")
    for a, b in zip(even, odd):                                 # the cut of the stream changes nothing
        assert a.start_sample == b.start_sample and np.array_equal(a.bits, b.bits)
        assert np.abs(np.array(a.rho) - np.array(b.rho)).max() <= 2e-9
        assert np.abs(a.Hs0 - b.Hs0).max() <= 1e-12 * np.abs(a.Hs0).max() and np.abs(a.He0 - b.He0).max() <= 1e-12 * np.abs(a.He0).max()
    # each transmission's bits are those of receive() on its stretch alone under the local rule
    rx = configured(OFDM.receiver, *CASES[name])
    rx.sync_rule = "local"
    for t, (lo, hi) in zip(even, sc["spans"]):
        bits, Hs, He = quiet(rx.receive, sc["stream"][lo - 3000: hi + 500])
        assert rx.no_packets == t.no_packets and np.array_equal(bits, t.bits)
        assert np.abs(Hs - t.Hs0).max() <= 1e-9 * np.abs(Hs).max()
        assert rx.sync_report["threshold"] == 0.3 and np.abs(np.array(rx.sync_report["rho"]) - np.array(t.rho)).max() <= 2e-9
    # ... and the reference's rule on the whole stream does not see the quiet transmission at all: the gap this closes
    rx.sync_rule = "global"
    bits, _, _ = quiet(rx.receive, sc["stream"])
    assert rx.no_packets == 3 and rx.sync_report is None and len(bits) == len(even[0].bits)
