"""The coded chain of the "QCLDPC-*" encodings in one place: settings and refusals, message bits -> coded bits, what the
demodulator must produce, its outputs -> LLRs, LLRs (or hard bits) -> message bits (through the per-codeword CRC where
`codeword_crc` is set), the decode report.  The façade (OFDM.py) builds a CodedChain from its public attributes at every
call and keeps what is the reference's: XOR, the coin-flip fill, the prints."""
from dataclasses import dataclass

import numpy as np
import torch

from .crc import CRC_BITS, CodewordCRC
from .engine import Engine
from .outer import OuterRS, from_transmitted, layout, packets_for, to_transmitted
from .pipeline import check_clock, correct_clock, fetch  # noqa: F401  (importable from here as before)

# channel coding beyond the reference's three encodings: the project's quasi-cyclic LDPC codes (ldpc.py), of block
# length CamG.ldpc_n = 1536 (the default), 3072 or 6144 coded bits
QCLDPC_ENCODINGS = {"QCLDPC-1/2": "1/2", "QCLDPC-2/3": "2/3", "QCLDPC-3/4": "3/4", "QCLDPC-5/6": "5/6"}
QCLDPC_LIFTING = {1536: 64, 3072: 128, 6144: 256}          # ldpc_n -> lifting size Z (24 block columns)


def decode_report(iters, status, outer=None, crc_bad=None):
    """`last_decode_report` from the decoder's iteration counts and the group statuses (host arrays; no statuses without
    an outer code).  With the outer code (G, R) it covers the members of the groups -- the rest is fill.  crc_bad: the
    per-codeword CRC flags where the codewords carry one (`iters` are the decoder's own counts, as they were before
    CodewordCRC.check): two more keys, the codewords that converged (iters > 0) on something whose CRC does not match."""
    iters, status = np.asarray(iters), np.asarray(status)
    if len(status):
        iters = iters[: len(status) * sum(outer)]
    failed = np.flatnonzero(iters < 0)
    rep = {"codewords": int(len(iters)), "inner_failed": int(len(failed)), "recovered": int(status[status > 0].sum()),
           "groups_failed": int((status < 0).sum()), "failed_codewords": failed.astype(np.int64)}
    if crc_bad is not None:
        wrong = np.flatnonzero((iters > 0) & (np.asarray(crc_bad)[: len(iters)] != 0))
        rep.update(crc_failed=int(len(wrong)), crc_failed_codewords=wrong.astype(np.int64))
    return rep


@dataclass
class CodedChain:
    """The façade's coding attributes as they are at one call, and the steps that depend on them."""
    encoding: str
    ldpc_n: int
    ldpc_max_iter: int
    llr_weighting: str
    interleave: bool
    fused_llr: bool
    outer_code: object
    per_packet: int                         # coded bits a packet carries
    make_code: object                       # (rate, device[, Z=Z]) -> QCLDPC: the façade's `_qcldpc_code`
    codeword_crc: bool = False              # the last 32 message bits of every codeword are the CRC of the others (crc.py)
    phase_tracking: bool = False            # receive(): Engine.track_phase on the equalised symbols, before the weights
    decoder_feedback: int = 0               # receive(): extra decoding passes at most, each re-equalised from the trusted codewords
    feedback_window: tuple = (2, 8)         # (half_symbols, half_bins) of Engine.feedback_equalise
    feedback_min_known: int = 4             # known symbols a window needs before its gain is used
    loading: tuple = None                   # adaptive bit loading (loading.py): the validated order per data carrier; per_packet then counts its bits
    denoise: tuple = None                   # receive() under `channel_denoising`: (denoise_threshold as the façade holds it, no_pilots)
    mimo_cancellation: int = 0              # receive_mimo(): extra passes at most, each detected again with the trusted codewords' bits known

    # ---- settings and their refusals -----------------------------------------------------------------------------------
    def rate(self):
        """Rate of a "QCLDPC-*" encoding, else None.  The interleaver and the codeword CRC exist on these encodings only."""
        rate = QCLDPC_ENCODINGS.get(self.encoding)
        self.check_loading()
        if self.interleave and rate is None:
            raise ValueError(f"interleave needs a 'QCLDPC-*' encoding, not {self.encoding!r}")
        if self.codeword_crc and rate is None:
            raise ValueError(f"codeword_crc needs a 'QCLDPC-*' encoding, not {self.encoding!r}")
        if self.phase_tracking and rate is None:
            raise ValueError(f"phase_tracking needs a 'QCLDPC-*' encoding, not {self.encoding!r}")
        if rate is None:
            self.outer()                        # (ValueError: the outer code exists on these encodings only)
        return rate

    def check_loading(self):
        """What a bit loading refuses: the steps that assume the context's uniform C mu layout (the interleaver's
        permutation, the carrier x symbol demapper, the fused kernel) or its one table's decisions (the tracker, the
        feedback's re-mapped symbols), and the XOR whitening, whose mask has the period of a uniform symbol."""
        if self.loading is None:
            return
        for name, on in (("interleave", self.interleave), ("llr_weighting 'noise2d'", self.llr_weighting == "noise2d"),
                         ("fused_llr", self.fused_llr), ("phase_tracking", self.phase_tracking),
                         ("decoder_feedback", self.decoder_feedback)):
            if on:
                raise ValueError(f"bit_loading: {name} works on the uniform layout of one table; switch it off")
        if self.encoding == "XOR":
            raise ValueError("bit_loading: encoding 'XOR' whitens with the period of a uniform symbol; use 'None' or 'QCLDPC-*'")

    def code(self, rate, device=None):
        """The code of this rate at block length `ldpc_n`, on `device` (None: the current one)."""
        Z = QCLDPC_LIFTING.get(self.ldpc_n)
        if Z is None:
            raise ValueError(f"ldpc_n must be one of {', '.join(map(str, QCLDPC_LIFTING))}, not {self.ldpc_n!r}")
        # (the default length keeps the (rate, device) call, which is what a stand-in for `_qcldpc_code` takes)
        return self.make_code(rate, device) if Z == 64 else self.make_code(rate, device, Z=Z)

    def outer(self):
        """(G, R) of `outer_code`, or None.  The outer code exists on the "QCLDPC-*" encodings only."""
        if self.outer_code is None:
            return None
        if QCLDPC_ENCODINGS.get(self.encoding) is None:
            raise ValueError(f"outer_code needs a 'QCLDPC-*' encoding, not {self.encoding!r}")
        try:
            G, R = (int(v) for v in self.outer_code)
        except (TypeError, ValueError):
            raise ValueError(f"outer_code must be None or (G, R), not {self.outer_code!r}")
        return G, R

    def outer_layout(self, F):
        """(cap, NG) for F packets: the whole codewords they hold and the outer-code groups among them (0 without one)."""
        gr = self.outer()
        return (F * self.per_packet // self.ldpc_n, 0) if gr is None else layout(F, self.per_packet, self.ldpc_n, *gr)

    def check_receive(self):
        """What receive() refuses before any GPU work -> (rate, fused: take the sample-to-LLR path)."""
        if self.llr_weighting not in ("csi", "noise", "noise2d"):
            raise ValueError(f"llr_weighting must be 'csi', 'noise' or 'noise2d', not {self.llr_weighting!r}")
        rate = self.rate()
        fused = rate is not None and bool(self.fused_llr)
        if fused and self.llr_weighting != "csi":
            raise ValueError(f"fused_llr needs llr_weighting 'csi': {self.llr_weighting!r} weights by the whole packet's "
                             "residuals, which the fused kernel does not have")
        if fused and self.phase_tracking:
            raise ValueError("phase_tracking needs fused_llr = False: the fused kernel never materialises the equalised "
                             "symbols the tracker works on")
        if self.check_denoise() is not None and fused:
            raise ValueError("channel_denoising needs fused_llr = False: the denoiser sits between the two-phase form's "
                             "launches, and the fused kernel is one launch")
        self.feedback()
        if self.decoder_feedback and rate is None:
            raise ValueError(f"decoder_feedback needs a 'QCLDPC-*' encoding, not {self.encoding!r}")
        if self.decoder_feedback and fused:
            raise ValueError("decoder_feedback needs fused_llr = False: the fused kernel never materialises the equalised "
                             "symbols the feedback corrects")
        return rate, fused

    def check_denoise(self):
        """The denoiser's threshold, or None where `channel_denoising` is off.  ValueError for a threshold that is not a
        finite number > 0 and for fewer than two pilot symbols per side."""
        if self.denoise is None:
            return None
        threshold = Engine.check_denoise(self.denoise[0])
        if self.denoise[1] < 2:
            raise ValueError(f"channel_denoising measures the noise from the pilot repeats: no_pilots >= 2, not {self.denoise[1]!r}")
        return threshold

    def feedback(self):
        """(passes, half_symbols, half_bins, min_known) of the decoder feedback; ValueError for a count that is not an
        integer >= 0 and, with a count > 0, for a window outside the ranges of Engine.feedback_equalise."""
        n = self.decoder_feedback
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError(f"decoder_feedback must be an integer >= 0 (the extra passes at most), not {n!r}")
        if not n:
            return 0, 0, 0, 1
        try:
            hs, hb = self.feedback_window
        except (TypeError, ValueError):
            raise ValueError(f"feedback_window must be (half_symbols, half_bins), not {self.feedback_window!r}")
        return (int(n),) + Engine.check_feedback_window(hs, hb, self.feedback_min_known)

    def cancellation(self):
        """The passes of `mimo_cancellation`; ValueError for a count that is not an integer >= 0."""
        n = self.mimo_cancellation
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError(f"mimo_cancellation must be an integer >= 0 (the extra passes at most), not {n!r}")
        return int(n)

    # ---- transmit side ---------------------------------------------------------------------------------------------------
    def encode(self, bits, rate, even=False):
        """Message bits -> coded bits (int64, host): zero padding to whole codewords, encoded on the GPU.  Outer code: the
        smallest packet count whose groups hold the message (the smallest even one under `even`: transmit_mimo sends
        packets in pairs, and the receiver lays the groups out over the packets it finds), zero padding to whole groups,
        then the parity codewords.
        `codeword_crc`: a codeword carries k = code.k - 32 of these bits and the CRC of them, parity codewords included."""
        code = self.code(rate)
        gr = self.outer()
        bits = bits.astype(np.uint8) & 1
        k = code.k - CRC_BITS if self.codeword_crc else code.k
        if gr is None:
            msg = np.concatenate([bits, np.zeros(-len(bits) % k, dtype=np.uint8)])
        else:
            G, R = gr
            rs = OuterRS(G, R, k)
            F = packets_for(len(bits), self.per_packet, code.n, k, G, R)
            NG = self.outer_layout(F + (F % 2 if even else 0))[1]
            data = torch.zeros(NG * G * k, dtype=torch.uint8)
            data[: len(bits)] = torch.from_numpy(bits)
            data = data.to(rs.device).reshape(NG, G, k)
            msg = to_transmitted(data, rs.encode(data).reshape(NG, R, k)).reshape(-1)
        if self.codeword_crc:
            msg = CodewordCRC(code.k).attach(torch.as_tensor(msg))
        return code.encode(torch.as_tensor(msg)).cpu().numpy().reshape(-1).astype(np.int64)

    # ---- receive side ----------------------------------------------------------------------------------------------------
    def llrs(self, eng, o, points):
        """Demodulator outputs -> (weighted max-log LLRs in coded order, {attribute name: rows for the host}: the SNR in dB
        of the noise weightings, 10 log10(Es / v') with the demapper's floor, `last_snr_db` [F, C], `last_symbol_snr_db`
        [F, D]; the tracker's `last_phase_track` [F, D, 2] and `last_phase_measured` [F, D] under `phase_tracking`)."""
        o, rows = self.track(eng, o)
        llr, snr = self.weigh(eng, o, points)
        rows.update(snr)
        return llr, rows

    def track(self, eng, o):
        """The tracker's part of `llrs`: -> (the outputs with the tracked symbols under `phase_tracking`, its rows)."""
        rows = {}
        if self.phase_tracking:
            # (a copy: the plots keep the untracked symbols)  `last_phase_track` [F, D, 2], `last_phase_measured` [F, D]
            o = dict(o)
            o["eq"], rows["last_phase_track"], rows["last_phase_measured"] = eng.track_phase(o["eq"], want_track=True)
        return o, rows

    def weigh(self, eng, o, points):
        """The weights' part of `llrs`, on o["eq"] as it is: -> (LLRs in coded order, the SNR rows)."""
        if self.loading is not None:
            return self.weigh_loaded(eng, o, self.llr_weighting)
        snr = {}
        if self.llr_weighting == "csi":
            llr = o["llr"] if "llr" in o else eng.soft_demap_csi(o["eq"], o["Hs"], o["He"])
        else:
            if self.llr_weighting == "noise":
                var, var_s = eng.noise_estimate(o["eq"]), None
                llr = eng.soft_demap_nw(o["eq"], var)
            else:
                var, var_s = eng.noise_estimate2(o["eq"])
                llr = eng.soft_demap_nw2(o["eq"], var, var_s, deinterleave=self.interleave)
            floor = 1e-6 * var.mean(dim=1, keepdim=True)
            es = float(np.mean(np.abs(points) ** 2))
            snr["last_snr_db"] = 10.0 * torch.log10(es / torch.maximum(var, floor))
            if var_s is not None:
                snr["last_symbol_snr_db"] = 10.0 * torch.log10(es / torch.maximum(var_s, floor))
        if self.interleave and self.llr_weighting != "noise2d":     # ("noise2d" de-interleaved inside its demapper)
            llr = eng.interleave(llr, inverse=True)
        return llr, snr

    def weigh_loaded(self, eng, o, weighting):
        """`weigh` under a bit loading: every carrier by its own table (Engine.soft_demap_loaded).  "noise" leaves
        `last_snr_db` [F, C] = 10 log10(1 / v') -- the tables have unit energy --, the carriers of order 0 included: their
        residual against the known pilot symbol is what lets a later allocation switch them back on."""
        ld = eng.loading(np.asarray(self.loading, dtype=np.uint8))
        if weighting == "csi":
            return eng.soft_demap_loaded(o["eq"], ld, Hs=o["Hs"], He=o["He"]), {}
        var = eng.noise_estimate_loaded(o["eq"], ld)
        llr = eng.soft_demap_loaded(o["eq"], ld, var=var)
        floor = 1e-6 * var.mean(dim=1, keepdim=True)
        return llr, {"last_snr_db": 10.0 * torch.log10(1.0 / torch.maximum(var, floor))}

    def check_diversity(self):
        """What receive_diversity() refuses before any GPU work -> rate."""
        if self.loading is not None:
            raise ValueError("receive_diversity: bit_loading is not combined (the combiner demaps by the context's one table)")
        if self.llr_weighting == "noise2d":
            raise ValueError("receive_diversity: llr_weighting must be 'csi' or 'noise'; 'noise2d' (per-symbol weights per "
                             "branch) is not combined")
        rate, _ = self.check_receive()
        for name in ("fused_llr", "phase_tracking", "decoder_feedback"):
            if getattr(self, name):
                raise ValueError(f"receive_diversity: {name} works on one recording; switch it off")
        return rate

    def check_mimo(self, who="receive_mimo", what="two streams"):
        """What receive_mimo() (and, as `who`, receive_stbc(), which sends `what` = "the space-time code") refuses before any
        GPU work -> rate.  The joint detector demaps by the context's one table and weights by the channel estimates
        themselves; the steps that work on one stream's equalised symbols have nothing to work on."""
        if self.loading is not None:
            raise ValueError(f"{who}: bit_loading is not detected jointly (the detector scans the context's one table)")
        if self.llr_weighting != "csi":
            raise ValueError(f"{who}: llr_weighting must be 'csi', not {self.llr_weighting!r}: the joint metric carries "
                             "the channel estimates as its weights")
        for name in ("fused_llr", "phase_tracking", "decoder_feedback"):
            if getattr(self, name):
                raise ValueError(f"{who}: {name} works on one stream's equalised symbols; switch it off")
        if self.interleave:
            raise ValueError(f"{who}: interleave is not supported with {what}; switch it off")
        return self.check_receive()[0]

    def combine(self, eng, outs, points, want="llr"):
        """Receive diversity: the per-branch demodulator outputs (B dicts with 'eq', 'Hs', 'He') -> (maximal-ratio combined
        LLRs in coded order -- or, want = "eq", the combined symbols for a hard decision --, {attribute name: rows for the
        host}).  Weights by `llr_weighting`: "csi" the |H^|^2 of each branch, "noise" 1 / the per-carrier variance
        Engine.noise_estimate measures on each branch, floored at 1e-6 of the packet's mean over all branches; the latter
        leaves `last_branch_snr_db` [B, F, C] = 10 log10(Es / floored variance) and `last_snr_db` [F, C] = 10 log10(Es
        sum_b w_b), the SNR after combining."""
        eqs, rows = [o["eq"] for o in outs], {}
        if self.llr_weighting == "csi":
            got = eng.combine_branches(eqs, Hs=[o["Hs"] for o in outs], He=[o["He"] for o in outs], want=(want,))[want]
        else:
            var = torch.stack([eng.noise_estimate(e) for e in eqs])                     # [B, F, C]
            got = eng.combine_branches(eqs, var=list(var), want=(want,))[want]
            vbar = var.mean(dim=(0, 2))[None, :, None]
            flat = ~(torch.isfinite(vbar) & (vbar > 0))
            floored = torch.maximum(var, 1e-6 * vbar)
            w = torch.where(flat, torch.ones_like(var), 1.0 / floored)
            w = torch.where(torch.isfinite(var) & torch.isfinite(w), w, torch.zeros_like(w))
            es = float(np.mean(np.abs(points) ** 2))
            rows["last_branch_snr_db"] = 10.0 * torch.log10(es / floored)
            rows["last_snr_db"] = 10.0 * torch.log10(es * w.sum(dim=0))
        if want == "llr" and self.interleave:
            got = eng.interleave(got, inverse=True)
        return got, rows

    def hard_llrs(self, bits, engine):
        """Received hard bits -> +-1 LLRs in coded order; `engine()` is asked for only to undo the interleaver."""
        b = np.asarray(bits)
        if self.interleave:
            if len(b) % self.per_packet:
                raise ValueError("interleave: decode() needs whole packets of packet_length * data_bits_per_symbol bits")
            b = engine().interleave(torch.from_numpy(np.ascontiguousarray(b, dtype=np.uint8)), inverse=True).cpu().numpy()
        return 1.0 - 2.0 * torch.as_tensor(np.asarray(b, dtype=np.float32))

    def decode(self, code, llr):
        """LLRs in coded order -> (message bits, iters [n_cw], group statuses, CRC flags [n_cw] or None) on the code's
        device: layered min-sum on every whole codeword, then the outer code rewrites up to R given-up members per group
        (no statuses without one).  `codeword_crc`: the CRC of every codeword is checked in between, the message bits are
        the payloads, and the outer code also rewrites the members that converged on something whose CRC does not match;
        the iteration counts returned are the decoder's own."""
        _, dec, iters, bad, erase = self.inner(code, llr[: llr.numel() // code.n * code.n])
        return self.outer_recover(dec, iters, bad, erase, llr.numel())

    def inner(self, code, llr):
        """Whole codewords' LLRs -> (the decoder's message rows [n_cw, code.k], the message bits they carry (the payloads
        under `codeword_crc`, else the rows themselves), iters, CRC flags or None, the counts the outer code erases by)."""
        full, iters = code.decode(llr, max_iter=self.ldpc_max_iter, want_iters=True)
        if not self.codeword_crc:
            return full, full, iters, None, iters
        dec, bad, erase = CodewordCRC(code.k, full.device).check(full, iters.clone())
        return full, dec, iters, bad, erase

    def outer_recover(self, dec, iters, bad, erase, n_llr):
        """`decode`'s second half: the outer code on the inner decoder's results for n_llr LLRs."""
        gr = self.outer()
        if gr is None:
            return dec.reshape(-1), iters, torch.empty(0, dtype=torch.int32, device=dec.device), bad
        if n_llr % self.per_packet:
            raise ValueError("outer_code: need whole packets of packet_length * data_bits_per_symbol bits")
        NG = self.outer_layout(n_llr // self.per_packet)[1]
        rows = NG * sum(gr)
        fixed, status = OuterRS(*gr, dec.shape[1], dec.device).recover(dec[:rows], erase[:rows])
        return from_transmitted(fixed, NG, gr[0]).reshape(-1), iters, status, bad

    def decode_feedback(self, eng, code, o, points):
        """receive() under `decoder_feedback`: tracker, weights and the first decode as without it; then up to
        `decoder_feedback` passes, each of which re-encodes the TRUSTED codewords (converged, and under `codeword_crc` with
        a matching CRC; their message rows are frozen from then on; every row goes through the encoder, the untrusted
        ones zeroed and masked rather than compacted), lays their coded bits and a per-bit mask out over the packets in
        transmitted order, has Engine.feedback_equalise measure the residual channel on those symbols of the
        ORIGINAL tracked `eq` and divide it out, weighs the result again and decodes the untrusted codewords alone.
        Passes are not cumulative (each starts from the same `eq` with more known symbols).  The loop ends when nothing
        is untrusted or a pass trusts nothing new; every pass, and the first decode, costs one small read-back (the
        codewords' flags).  The loop itself is `decode_again`, which decode_cancel shares.  The outer code then sees the
        final bits and erasures.
        -> (message bits, iters, group statuses, CRC flags or None, the host rows of `llrs`, {"feedback_passes",
        "feedback_recovered"})."""
        passes, hs, hb, min_known = self.feedback()
        o, rows = self.track(eng, o)
        llr, snr = self.weigh(eng, o, points)
        last = {"snr": snr}

        def again(full, trusted, untrusted):
            bits, known = self.known_planes(eng, code, full, trusted, llr.numel() // self.per_packet)
            fb = dict(o)
            fb["eq"] = eng.feedback_equalise(o["eq"], bits, known, hs, hb, min_known)
            new, last["snr"] = self.weigh(eng, fb, points)
            return new
        dec, iters, bad, erase, done, recovered = self.decode_again(code, llr, passes, again)
        rows.update(last["snr"])
        bits, iters, status, bad = self.outer_recover(dec, iters, bad, erase, llr.numel())
        return bits, iters, status, bad, rows, {"feedback_passes": done, "feedback_recovered": recovered}

    def decode_cancel(self, eng, code, llr, detect):
        """receive_mimo() under `mimo_cancellation`: the first decode of the joint detector's `llr` as without it; then up
        to `mimo_cancellation` passes of successive interference cancellation.  The bookkeeping is decode_feedback's
        (`decode_again`): a pass re-encodes the TRUSTED codewords and lays their coded bits and a per-bit mask out over the
        packets in transmitted order, which is the layout of the detector's LLRs.  `detect(pairs, bits, known)` -- the
        façade's: the data symbols' spectra of those packet pairs again, Engine.mimo_detect_known on them under the call's
        weights -- is asked for the LLRs [len(pairs), 2 per_packet] of the packet pairs (ascending, a host array) that hold
        a bit of an untrusted codeword, given those pairs' rows of the two planes; the untrusted codewords alone are
        decoded from them.  Passes are cumulative only in what is known: each detects from the same spectra.  One small
        read-back per pass.  -> (message bits, iters, group statuses, CRC flags or None, {"cancel_passes",
        "cancel_recovered"})."""
        llr = llr.reshape(-1)                                   # (the façade's own buffer: the passes overwrite their pairs' rows)
        n, pair = code.n, 2 * self.per_packet

        def again(full, trusted, untrusted):
            bits, known = self.known_planes(eng, code, full, trusted, llr.numel() // self.per_packet)
            lo, hi = untrusted * n // pair, ((untrusted + 1) * n - 1) // pair     # (first and last pair of each codeword)
            pairs = np.unique(np.concatenate([np.arange(a, b + 1) for a, b in zip(lo, hi)]))
            at = torch.from_numpy(pairs).to(llr.device)
            llr.view(-1, pair)[at] = detect(pairs, bits.view(-1, pair)[at], known.view(-1, pair)[at]).reshape(len(pairs), pair)
            return llr
        dec, iters, bad, erase, done, recovered = self.decode_again(code, llr, self.cancellation(), again)
        bits, iters, status, bad = self.outer_recover(dec, iters, bad, erase, llr.numel())
        return bits, iters, status, bad, {"cancel_passes": done, "cancel_recovered": recovered}

    def known_planes(self, eng, code, full, trusted, F):
        """The message rows `full` [n_cw, code.k] and the 0 / 1 flags `trusted` [n_cw] -> (bits, known): uint8 [F, per_packet]
        in transmitted order, the trusted codewords re-encoded (every row goes through the encoder, the untrusted ones
        zeroed and masked rather than compacted) and one mask byte per coded bit."""
        n_cw = full.shape[0]
        planes = []
        for rows_u8 in (code.encode(full * trusted[:, None]), trusted[:, None].expand(n_cw, code.n)):
            plane = torch.zeros((F, self.per_packet), dtype=torch.uint8, device=full.device)
            plane.view(-1)[: n_cw * code.n] = rows_u8.reshape(-1)
            planes.append(eng.interleave(plane, inverse=False) if self.interleave else plane)
        return planes

    def decode_again(self, code, llr, passes, again):
        """What decode_feedback and decode_cancel share: the first decode of the whole codewords of `llr` (coded order), then
        up to `passes` more.  A codeword is TRUSTED once it converged and, under `codeword_crc`, its CRC matches; its
        message row is frozen from then on.  A pass asks `again(message rows [n_cw, code.k], trusted flags uint8 [n_cw],
        the untrusted codewords' numbers (host, ascending))` for new LLRs in coded order and decodes the untrusted
        codewords alone.  The loop ends when nothing is untrusted or a pass trusts nothing new; every pass, and the first
        decode, costs one small read-back (the flags).  -> (the message bits per codeword, iters, CRC flags or None, the
        counts the outer code erases by, the passes run, the codewords they came to trust)."""
        n_cw = llr.numel() // code.n
        full, dec, iters, bad, erase = self.inner(code, llr[: n_cw * code.n])
        first = None
        done = 0
        while True:
            untrusted = np.flatnonzero(erase.cpu().numpy() <= 0)    # (the read-back: a codeword is trusted once erase > 0)
            left = len(untrusted)
            first = left if first is None else first
            if done and left == last:
                break
            last = left
            if done == passes or left == 0:
                break
            llr = again(full, (erase > 0).to(torch.uint8), untrusted)
            at = torch.from_numpy(untrusted).to(full.device)
            sub = llr[: n_cw * code.n].reshape(n_cw, code.n)[at]
            full_u, dec_u, iters_u, bad_u, erase_u = self.inner(code, sub)
            full[at] = full_u
            iters[at] = iters_u
            if self.codeword_crc:
                dec[at], bad[at], erase[at] = dec_u, bad_u, erase_u
            done += 1
        return dec, iters, bad, erase, done, first - last
