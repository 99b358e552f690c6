"""LiveReceiver: receive while the stream is still arriving.

The reference's sync rule needs the whole recording (its threshold is relative to the global maximum); the self-normalised
rule (Engine.detect_chunk / detect_decide) does not, so a stream can be fed block by block:

    live = LiveReceiver(rx)
    for block in source:                 # any block sizes, the storage of the first block throughout
        for t in live.feed(block):       # the transmissions that ENDED inside this block
            t.bits, t.start_sample, t.no_packets, t.rho, t.decode_report, t.Hs0, t.He0
    live.flush()                         # end of stream: what can still be closed

`Segmenter` is the state machine between the two (detections in, closed transmissions out); it works on integers and makes
no GPU call.  Whatever a listener must survive -- a lone chirp, a transmission that never ends, a packet cut off by the end
of the stream, a transmission that fails to decode -- becomes an entry of `live.events`, never an exception.

With `rx.input_rate` set the blocks are taken at that rate: every block is converted to fs as far as its outputs are final
(Engine.resample_stream on the stream's own indices, with the input samples the next outputs still read carried over), so
what the detector and the decoder see is byte for byte the whole stream converted at once, whatever the block sizes; every
index reported stays in fs numbering, and `Transmission.start_input_sample` is the index in the stream as it was fed."""
import contextlib
import io
import math
from dataclasses import dataclass

import numpy as np
import torch

from .engine import ListOverflow
from .pipeline import plan_receive

END = (1 << 62) - 1                                             # "the stream has ended" (INT64_MAX / 2, gf3_detect_decide)


class Segmenter:
    """Detections -> transmissions in the reference's format [chirp|packet] ... [chirp].  A detection opens a transmission; a
    further one extends it if it follows the previous one by a packet's length: no earlier than frame_len - slack (a packet
    lies between two chirps of one transmission, so a chirp that comes sooner belongs to the NEXT transmission and the
    previous one was a terminating chirp) and no later than `reach` = frame_len + max_gap.  When no such detection can
    arrive any more, the last one was the terminating chirp and the transmission is closed."""

    def __init__(self, frame_len, max_gap, slack=0):
        self.near = int(frame_len) - int(slack)
        self.reach = int(frame_len) + int(max_gap)
        self.open = []                                          # the detections of the open transmission

    def push(self, detections, horizon):
        """detections: new ones, ascending, all behind the ones pushed before.  horizon: every detection with an index below
        it is known by now.  -> the transmissions this closes, each the list of its detections."""
        closed = []
        for d in detections:
            d = int(d)
            if self.open and not self.near <= d - self.open[-1] <= self.reach:
                closed.append(self.open)
                self.open = []
            self.open.append(d)
        if self.open and horizon > self.open[-1] + self.reach:
            closed.append(self.open)
            self.open = []
        return closed

    def force(self):
        """Close the open transmission as it stands -> its detections."""
        out, self.open = self.open, []
        return out


@dataclass
class Transmission:
    bits: np.ndarray                                            # what rx.receive returns for it
    start_sample: int                                           # the first packet's first sample, in the stream's numbering
    no_packets: int
    rho: list                                                   # the coefficient of every detection, the terminating chirp's last
    decode_report: object                                       # rx.last_decode_report of its decode
    Hs0: np.ndarray
    He0: np.ndarray
    start_input_sample: int = None                              # start_sample in the numbering of the stream as it was fed


class LiveReceiver:
    def __init__(self, rx, max_gap=None, max_transmission_samples=1 << 27):
        """rx: a receiver; every receive option on it means what it means in rx.receive().  max_gap: samples that may lie
        between a packet's end and the next chirp of the same transmission (default: one chirp length).  A transmission
        longer than max_transmission_samples is closed where it stands.  Whatever rx.receive() under sync_rule = "local"
        refuses is refused here, once."""
        self.rx = rx
        self.Lc = int(rx.chirp_length)
        self.body = (2 * rx.no_pilots + rx.packet_length) * (rx.cp_length + rx.ofdm_symbol_size)
        self.max_gap = self.Lc if max_gap is None else int(max_gap)
        self.max_samples = int(max_transmission_samples)
        self.seg = Segmenter(self.Lc + self.body, self.max_gap, slack=rx.cp_length)
        self.events = []
        with self._local():
            plan = plan_receive(rx, rx._chain(), [self.max_samples], False, False)
        self.tau = plan.detect
        self.rate = plan.rates[0] if plan.rates else None       # (input rate, half_taps) of the fed stream, or None
        self.r = 1.0 if self.rate is None else self.rate[0] / float(rx.fs)
        self.n_fed = self.raw_base = self.n_converted = 0       # input samples fed; stream index of raw[0]; outputs made so far
        self.eng = None
        self.n_seen = self.n_done = self.base = 0               # samples fed; lags through detect_chunk; stream index of buf[0]
        self.decided = -END                                     # final_below of the last decision
        self.rho_of = {}                                        # coefficient of every detection still held by the segmenter

    @contextlib.contextmanager
    def _local(self):
        kept, self.rx.sync_rule = self.rx.sync_rule, "local"
        try:
            yield
        finally:
            self.rx.sync_rule = kept

    def _start(self, block):
        dtype = block.dtype if isinstance(block, np.ndarray) else torch.empty(0, dtype=block.dtype).numpy().dtype
        dtype = dtype if dtype in (np.float64, np.float32, np.int16, np.uint8) else np.dtype("float64")
        self.raw_dtype = dtype
        if self.rate is not None:                               # the conversion's output type, as in rx.receive()
            dtype = np.dtype("float64") if dtype == np.float64 else np.dtype("float32")
        self.eng = eng = self.rx._engine(dtype)
        self.raw = torch.empty((0,), dtype=torch.from_numpy(np.empty(0, self.raw_dtype)).dtype, device=eng.device)
        self.buf = torch.empty((0,), dtype=eng.cfg.in_dtype, device=eng.device)
        self.vrun = torch.zeros((1,), dtype=torch.float64, device=eng.device)
        self.idx = torch.empty((0,), dtype=torch.int64, device=eng.device)
        self.rho = torch.empty((0,), dtype=torch.float64, device=eng.device)

    def feed(self, block):
        """Take the next samples of the stream -> the transmissions that ended inside them (a list, often empty)."""
        if self.eng is None:
            self._start(block)
        if self.rate is not None:
            return self._feed(self._convert(block, final=False))
        return self._feed(self.eng._samples(block).reshape(-1))

    def _convert(self, block, final):
        """The next input samples (None: none) -> the samples at fs that they make final (final: the stream has ended -- all
        that are left, the taps behind the end reading zeros)."""
        if block is not None:
            block = torch.as_tensor(block).reshape(-1)
            self.raw = torch.cat([self.raw, block.to(self.raw.dtype).to(self.eng.device)])
            self.n_fed += block.numel()
        r, half_taps = self.r, self.rate[1]
        upto = self.eng.stream_outputs(self.n_fed, r, half_taps, final=final)
        y = self.eng.resample_stream(self.raw, r, half_taps, in_origin=self.raw_base, j0=self.n_converted,
                                     n_out=max(upto - self.n_converted, 0))
        self.n_converted = max(upto, self.n_converted)
        reach = int(math.ceil(half_taps * r)) if r > 1.0 else half_taps
        keep = max(int(math.floor(float(self.n_converted) * r)) - reach + 1, self.raw_base)     # the first sample the next output reads
        if keep > self.raw_base:
            self.raw, self.raw_base = self.raw[keep - self.raw_base:].clone(), keep
        return y

    def _feed(self, x):
        """feed() on samples at fs in the engine's storage."""
        if x.numel() == 0:
            return []
        self.buf = torch.cat([self.buf, x])
        self.n_seen += x.numel()
        lo = max(self.base, self.n_done - (self.Lc - 1))        # the new lags' windows begin here
        view = self.buf[lo - self.base:]
        if view.numel() < 3:
            return []
        cap = 1024
        while True:
            try:
                idx, rho = self.eng.detect_chunk(view, self.n_done - lo, self.n_seen - lo, lo, self.vrun, self.tau, cap)
                break
            except ListOverflow as e:
                cap = e.wanted
        self.n_done = self.n_seen
        self.idx, self.rho = torch.cat([self.idx, idx]), torch.cat([self.rho, rho])
        out = self._decide(self.n_seen - 1)
        if self.seg.open and self.n_seen - self.seg.open[0] > self.max_samples:
            dets = self.seg.force()
            self.events.append({"kind": "forced_close", "start_sample": dets[0] + 2, "samples": self.n_seen - dets[0]})
            out += self._close([dets])
        keep = min([self.n_seen - 2 * self.Lc] + ([self.seg.open[0] - self.Lc] if self.seg.open else []))
        if keep > self.base:
            self.buf, self.base = self.buf[keep - self.base:].clone(), keep
        return out

    def flush(self):
        """The stream has ended: decide what was withheld, close what is open -> the transmissions that gives.  A transmission
        still open with more than max_gap samples behind its last chirp is reported as a cut-off packet."""
        if self.eng is None:
            return []
        out = self._feed(self._convert(None, final=True)) if self.rate is not None else []
        return out + self._flush()

    def _flush(self):
        was_open = bool(self.seg.open) or bool(self.idx.numel())
        out = self._decide(END, at_end=was_open)
        self.idx, self.rho = self.idx[:0], self.rho[:0]
        return out

    def _decide(self, final_below, at_end=False):
        peaks = self.eng.detect_decide(self.idx, self.rho, final_below)
        new = peaks[peaks + self.Lc > self.decided]             # (the others were emitted by an earlier decision)
        rho = self.rho[torch.searchsorted(self.idx, new)]
        self.decided = final_below
        new, rho = new.cpu().tolist(), rho.cpu().tolist()
        self.rho_of.update(zip(new, rho))
        keep = self.idx + 2 * self.Lc > final_below             # the entries that can still change a decision
        self.idx, self.rho = self.idx[keep], self.rho[keep]
        closed = self.seg.push(new, final_below - self.Lc + 1)
        if at_end and closed and self.n_seen - (closed[-1][-1] + 2) > self.max_gap:
            self.events.append({"kind": "cut_packet", "start_sample": closed[-1][-1] + 2,
                                "samples": self.n_seen - (closed[-1][-1] + 2)})
        return self._close(closed)

    def _close(self, closed):
        out = []
        for dets in closed:
            rho = [self.rho_of.pop(d) for d in dets]
            starts = [d + 2 for d in dets[:-1]]
            while starts and starts[-1] + self.body > self.n_seen:      # (only a forced close or the end of the stream can cut one)
                self.events.append({"kind": "cut_packet", "start_sample": starts.pop(), "samples": self.n_seen - dets[-2] - 2})
                dets = dets[:-1]
            if not starts:
                self.events.append({"kind": "lone_chirp", "index": dets[0], "rho": rho[0]})
                continue
            x = self.buf[starts[0] - self.base: starts[-1] + self.body - self.base]
            peaks = torch.tensor([d - starts[0] for d in dets], dtype=torch.int64, device=self.eng.device)
            try:
                with self._local(), contextlib.redirect_stdout(io.StringIO()):
                    bits, Hs0, He0 = self.rx._receive(None, False, False,
                                                      located=(x, peaks, torch.tensor(rho[: len(dets)], dtype=torch.float64,
                                                                                      device=self.eng.device)))
            except Exception as e:                              # (a listener survives a transmission it cannot decode)
                self.events.append({"kind": "decode_failed", "start_sample": starts[0], "packets": len(starts),
                                    "error": f"{type(e).__name__}: {e}"})
                continue
            out.append(Transmission(bits, starts[0], len(starts), rho, self.rx.last_decode_report, Hs0, He0,
                                    int(math.floor(starts[0] * self.r))))
        return out
