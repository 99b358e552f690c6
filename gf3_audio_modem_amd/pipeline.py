"""What receive() and receive_diversity() share around the decode stage ("The receive pipeline"): the plan --
every refusal of a receive call, in one order, before any GPU work --, the clock correction of one recording, the one
demodulator call, and `fetch`, the one small device-to-host copy a receive call ends with."""
from typing import NamedTuple

import numpy as np
import torch

from .engine import Engine

PIECEWISE_ABOVE = 1 << 27                                   # samples: a longer recording is taken from host memory piece by piece
PIECEWISE_CHUNK = 1 << 25                                   # samples per piece where `host_chunk_samples` names none
RATE_RANGE = (24000.0, 192000.0)                           # sampling rates `input_rate` / `output_rate` take, in Hz
CLOCK_MAX_PPM = 2000.0                                      # |eps| <= 2e-3: beyond it gf3_resample_frames copies the body
_HOST = "the piece-wise host path of long recordings (or host_chunk_samples)"
_LOCAL = "sync_rule 'local': {host} decides by the reference's global rule; feed the stream to a LiveReceiver"


def fetch(tensors):
    """{name: tensor}, all on one device -> {name: NumPy array of the tensor's shape and dtype}, through ONE
    concatenation, ONE copy (pinned and non-blocking from a GPU) and ONE stream synchronisation.  The values travel as
    float64: complex ones as (re, im) pairs, integers converted, which is exact for the int32 values sent here."""
    parts = [(torch.view_as_real(t) if t.is_complex() else t).reshape(-1).to(torch.float64) for t in tensors.values()]
    small = torch.cat(parts)
    host = torch.empty(small.numel(), dtype=torch.float64, pin_memory=small.is_cuda)
    host.copy_(small, non_blocking=True)
    if small.is_cuda:
        torch.cuda.current_stream(small.device).synchronize()
    out, at = {}, 0
    for (name, t), part in zip(tensors.items(), parts):
        a = host[at: at + part.numel()].numpy().copy()
        at += part.numel()
        a = a.view(np.complex128) if t.is_complex() else a
        out[name] = a.astype(torch.empty(0, dtype=t.dtype).numpy().dtype, copy=False).reshape(tuple(t.shape))
    return out


def check_clock(clock_correction, clock_taps):
    """What `clock_correction` / `clock_taps` refuse before any GPU work -> None (off), or ("auto" | the offset in ppm as a float,
    half_taps).  ValueError for another string, a value that is not a finite number of at most 2000 ppm in magnitude, and a
    tap count other than 32 or 64."""
    if clock_correction is None:
        return None
    if isinstance(clock_taps, bool) or clock_taps not in (32, 64):
        raise ValueError(f"clock_taps must be 32 or 64, not {clock_taps!r}")
    if isinstance(clock_correction, str):
        if clock_correction != "auto":
            raise ValueError(f"clock_correction must be None, 'auto' or a number in ppm, not {clock_correction!r}")
        return "auto", int(clock_taps) // 2
    try:
        ppm = float(clock_correction)
        ok = not isinstance(clock_correction, bool) and np.isfinite(ppm) and abs(ppm) <= CLOCK_MAX_PPM
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"clock_correction must be None, 'auto' or a finite number of at most {CLOCK_MAX_PPM:.0f} ppm in "
                         f"magnitude, not {clock_correction!r}")
    return ppm, int(clock_taps) // 2


def check_rate(rate, rate_taps, fs, name="input_rate"):
    """What `input_rate` / `output_rate` and `rate_taps` refuse before any GPU work -> None (off, or the rate is fs itself), or
    (the rate in Hz as a float, half_taps).  ValueError for a value that is not a finite number in [24000, 192000] and for a
    tap count other than 32 or 64."""
    if rate is None:
        return None
    if isinstance(rate_taps, (bool, np.bool_)) or rate_taps not in (32, 64):
        raise ValueError(f"rate_taps must be 32 or 64, not {rate_taps!r}")
    number = isinstance(rate, (int, float, np.integer, np.floating)) and not isinstance(rate, (bool, np.bool_))
    if not number or not RATE_RANGE[0] <= float(rate) <= RATE_RANGE[1]:     # (NaN fails both comparisons)
        raise ValueError(f"{name} must be None or a finite number of samples per second in [{RATE_RANGE[0]:.0f}, {RATE_RANGE[1]:.0f}], "
                         f"not {rate!r}")
    return None if float(rate) == float(fs) else (float(rate), int(rate_taps) // 2)


def check_input_rates(rx, count, diversity):
    """`input_rate` of a receive call on `count` recordings -> None (no recording is converted), or a tuple with check_rate's
    answer for every recording.  receive_diversity() also takes a sequence with one rate per recording.  ValueError for
    what check_rate refuses, a sequence of another length (or any sequence under receive()), and a rate whose Nyquist
    frequency the top data carrier reaches: nothing could decode it."""
    rate = rx.input_rate
    if rate is None:
        return None
    if isinstance(rate, (list, tuple, np.ndarray)):
        if not diversity:
            raise ValueError(f"input_rate must be None or one number for receive(), not {rate!r}")
        if len(rate) != count:
            raise ValueError(f"input_rate holds {len(rate)} rates for {count} recordings")
        rates = [check_rate(v, rx.rate_taps, rx.fs) for v in rate]
    else:
        rates = [check_rate(rate, rx.rate_taps, rx.fs)] * count
    top = float(np.max(rx.data_carriers)) * float(rx.fs) / rx.ofdm_symbol_size
    for v in rates:
        if v is not None and top >= v[0] / 2.0:
            raise ValueError(f"input_rate {v[0]:g}: the top data carrier lies at {top:.0f} Hz, at or above half that rate; "
                             "nothing could decode it")
    return tuple(rates) if any(v is not None for v in rates) else None


def check_sync_rule(sync_rule, detect_threshold):
    """What `sync_rule` / `detect_threshold` refuse before any GPU work -> None under "global" (the reference's rule), the
    threshold as a float under "local" (Engine.detect_stream).  ValueError for another rule and for a threshold that is not a
    finite number inside (0, 1)."""
    if not isinstance(sync_rule, str) or sync_rule not in ("global", "local"):
        raise ValueError(f"sync_rule must be 'global' or 'local', not {sync_rule!r}")
    tau = Engine.check_detect(detect_threshold)
    return tau if sync_rule == "local" else None


class ReceivePlan(NamedTuple):
    """What one receive call does, decided before any GPU work; everything after `plan_receive` reads these and checks nothing again."""
    chain: object                           # the CodedChain of this call
    rate: object                            # rate of a "QCLDPC-*" encoding, else None
    fused: bool                             # take the sample-to-LLR demodulator (never with the plots, which need eq)
    blanking: object                        # (threshold, guard) of Engine.blank_impulses, or None
    clock: object                           # check_clock's answer, or None
    denoise: object                         # the denoiser's threshold, or None
    plots: bool
    piecewise: bool                         # the recording is taken from host memory piece by piece (Engine.receive_host)
    chunk: int                              # samples per piece
    detect: object = None                   # the threshold of the self-normalised detection (sync_rule "local"), or None
    rates: object = None                    # check_input_rates' answer: per recording None or (input rate, half_taps), or None
    advance: int = 0                        # receive_mimo: samples every packet start is moved back by (`mimo_advance`)
    joint_noise: bool = False               # receive_mimo, receive_stbc: pilot-measured weights (`joint_weighting` = "noise")
    cancel: int = 0                         # receive_mimo: passes of decoder-driven cancellation at most (`mimo_cancellation`)
    window: int = 0                         # samples of the receive window's ramp (`receive_window`), 0: no windowing stage


def check_mimo_pilots(no_pilots):
    """The pilot cover of 2 x 2 spatial multiplexing needs an even number of pilot symbols, at least 2 (ValueError)."""
    if isinstance(no_pilots, (bool, np.bool_)) or not isinstance(no_pilots, (int, np.integer)) or no_pilots < 2 or no_pilots % 2:
        raise ValueError(f"spatial multiplexing covers the pilots in pairs: no_pilots must be even and >= 2, not {no_pilots!r}")
    return int(no_pilots)


def check_advance(advance, cp_length):
    """`mimo_advance` -> the samples as an int; ValueError unless it is an integer in [0, cp_length]."""
    if isinstance(advance, (bool, np.bool_)) or not isinstance(advance, (int, np.integer)) or not 0 <= advance <= cp_length:
        raise ValueError(f"mimo_advance must be an integer number of samples in [0, cp_length = {cp_length}], not {advance!r}")
    return int(advance)


def check_joint_weighting(joint_weighting, no_pilots, who):
    """`joint_weighting` -> True under "noise" (Engine.mimo_pilot_noise, joint_noise_weights), False under "csi".  ValueError
    for another value, and for "noise" with fewer than 4 pilot symbols: the two covers take two of them per carrier and the
    noise is measured on the rest."""
    if not isinstance(joint_weighting, str) or joint_weighting not in ("csi", "noise"):
        raise ValueError(f"{who}: joint_weighting must be 'csi' or 'noise', not {joint_weighting!r}")
    if joint_weighting == "noise" and no_pilots < 4:
        raise ValueError(f"{who}: joint_weighting = 'noise' measures the noise on the pilot symbols the two covers leave over: "
                         f"no_pilots must be >= 4, not {no_pilots!r}")
    return joint_weighting == "noise"


def check_cancellation(chain, rate, who, cancels):
    """`mimo_cancellation` -> the passes as an int.  ValueError for a value that is not an integer >= 0, for a value > 0
    under an encoding without codewords to trust, and (cancels False: the space-time code) for any value > 0."""
    passes = chain.cancellation()
    if passes and not cancels:
        raise ValueError(f"{who}: mimo_cancellation cancels one stream of two out of the other; the pair of the space-time code "
                         "decouples and there is nothing to cancel; leave it at 0")
    if passes and rate is None:
        raise ValueError(f"{who}: mimo_cancellation needs a 'QCLDPC-*' encoding, not {chain.encoding!r}: the decoded codewords "
                         "are what is cancelled")
    return passes


def plan_mimo(rx, chain, lengths, plots, who="receive_mimo", what="two streams", verb="separates", cancels=True):
    """The plan of receive_mimo() on recordings of `lengths` samples, in plan_receive's manner and order: the pilot cover's
    and the coded chain's own refusals (CodedChain.check_mimo), the values of the joint weighting, the advance, the clock
    correction, the sync rule, the input rate and the receive window (ValueError), then what has no path
    (NotImplementedError).  No GPU work.
    (plan_stbc names itself in `who` and, with cancels = False, refuses `mimo_cancellation`.)"""
    check_mimo_pilots(rx.no_pilots)
    rate = chain.check_mimo(who, what)
    joint_noise = check_joint_weighting(rx.joint_weighting, rx.no_pilots, who)
    advance = check_advance(rx.mimo_advance, rx.cp_length)
    clock = check_clock(rx.clock_correction, rx.clock_taps)
    detect = check_sync_rule(rx.sync_rule, rx.detect_threshold)
    rates = check_input_rates(rx, len(lengths), True)
    cancel = check_cancellation(chain, rate, who, cancels)
    window = Engine.check_window(rx.receive_window, rx.cp_length)
    if advance + window > rx.cp_length:
        raise ValueError(f"{who}: mimo_advance + receive_window = {advance} + {window} samples exceed cp_length = {rx.cp_length}: "
                         "nothing of the prefix would be left")
    chunk = getattr(rx, "host_chunk_samples", None)
    piecewise = bool(chunk or any(n > PIECEWISE_ABOVE for n in lengths))
    no_path = ((rx.impulse_blanking, f"{who}: impulse_blanking is not applied; blank each recording's samples with "
                                     "Engine.blank_impulses first"),
               (rx.channel_denoising, f"{who}: channel_denoising cleans one column of the channel; the two covers have "
                                      "no denoiser"),
               (plots, f"{who}: no plots; receive() one stream for them"),
               (piecewise, f"{who}: {{host}} {verb} nothing; receive shorter recordings"))
    for on, why in no_path:
        if on:
            raise NotImplementedError(why.format(host=_HOST))
    return ReceivePlan(chain, rate, False, None, clock, None, False, False, int(chunk or PIECEWISE_CHUNK), detect, rates, advance,
                       joint_noise, cancel, window)


def check_stbc_length(packet_length):
    """The Alamouti code pairs the data symbols: an even packet_length (ValueError)."""
    if packet_length % 2:
        raise ValueError(f"the space-time code pairs the data symbols: packet_length must be even, not {packet_length!r}")
    return int(packet_length)


def plan_stbc(rx, chain, lengths, plots):
    """The plan of receive_stbc(): plan_mimo's checks under its own name (a `mimo_cancellation` > 0 refused: nothing to
    cancel), and the pairing of the data symbols."""
    plan = plan_mimo(rx, chain, lengths, plots, "receive_stbc", "the space-time code", "decodes", cancels=False)
    check_stbc_length(rx.packet_length)
    return plan


def plan_receive(rx, chain, lengths, plots, diversity):
    """The plan of receive() (diversity False) or receive_diversity() on recordings of `lengths` samples, from the
    receiver's attributes as they are now and its CodedChain.  Every refusal of a receive call is raised here, in this order:
    the coded chain's own (CodedChain.check_receive / check_diversity: ValueError), the values of the blanking and the
    clock correction, of the sync rule, of the input rate and of the receive window (ValueError), then what has no path
    (NotImplementedError)."""
    chunk = getattr(rx, "host_chunk_samples", None)
    piecewise = not plots and bool(chunk or any(n > PIECEWISE_ABOVE for n in lengths))
    if diversity:
        rate, fused, blanking = chain.check_diversity(), False, None
        clock = check_clock(rx.clock_correction, rx.clock_taps)
        detect = check_sync_rule(rx.sync_rule, rx.detect_threshold)
        rates = check_input_rates(rx, len(lengths), True)
        window = Engine.check_window(rx.receive_window, rx.cp_length)
        no_path = ((rx.impulse_blanking, "receive_diversity: impulse_blanking is not combined; blank each recording's samples "
                                         "with Engine.blank_impulses first"),
                   (plots, "receive_diversity: no plots; receive() one recording for them"),
                   (piecewise, "receive_diversity: {host} combines nothing; receive shorter recordings"),
                   (detect and piecewise, _LOCAL),
                   (rates and piecewise, "input_rate: {host} has no rate conversion; receive shorter recordings"),
                   (window and piecewise, "receive_window: {host} has no windowing pass; receive shorter recordings"))
    else:
        rate, fused = chain.check_receive()
        blanking = Engine.check_blanking(rx.blanking_threshold, rx.blanking_guard) if rx.impulse_blanking else None
        clock = check_clock(rx.clock_correction, rx.clock_taps)
        detect = check_sync_rule(rx.sync_rule, rx.detect_threshold)
        rates = check_input_rates(rx, len(lengths), False)
        window = Engine.check_window(rx.receive_window, rx.cp_length)
        loaded = chain.loading is not None
        no_path = ((chain.denoise and piecewise, "channel_denoising: {host} has no denoising pass; receive shorter recordings"),
                   (loaded and plots, "bit_loading: the plots draw one constellation; receive with graph_output = False"),
                   (loaded and piecewise, "bit_loading: {host} decides by the context's one table; receive shorter recordings"),
                   (blanking and piecewise, "impulse_blanking: {host} has no blanking pass; receive shorter recordings"),
                   (clock and piecewise, "clock_correction: {host} has no resampling pass; receive shorter recordings"),
                   (rate is not None and piecewise, "encoding {encoding!r}: {host} has no soft-decision decoding; "
                                                    "receive shorter recordings"),
                   (detect and piecewise, _LOCAL),
                   (rates and piecewise, "input_rate: {host} has no rate conversion; receive shorter recordings"),
                   (window and piecewise, "receive_window: {host} has no windowing pass; receive shorter recordings"))
    for on, why in no_path:
        if on:
            raise NotImplementedError(why.format(host=_HOST, encoding=chain.encoding))
    denoise = None if chain.denoise is None else float(chain.denoise[0])       # (validated by the chain's checks above)
    return ReceivePlan(chain, rate, fused and not plots, blanking, clock, denoise, bool(plots), piecewise,
                       int(chunk or PIECEWISE_CHUNK), detect, rates, window=window)


def convert_rate(eng, r, rate, fs):
    """One recording (a host array of any storage type) taken at `rate` = check_rate's answer -> the engine's samples at fs:
    uploaded as it is and converted whole (Engine.resample_stream with r = rate / fs)."""
    return eng.resample_stream(torch.from_numpy(r), rate[0] / float(fs), half_taps=rate[1])


def correct_clock(eng, x, starts, clock):
    """The clock correction of one recording: clock = check_clock's answer (not None).  "auto": one demodulation for the
    slopes, eps per packet (Engine.clock_offset), and the median of the finite estimates for every packet -- a sound card
    has one clock, and one noisy packet must not get its own rate.  A number: that many ppm, no first pass.
    -> (rows, offsets: what the demodulator takes in place of (x, starts), status int32 [F]: non-zero for a packet that runs
    past the recording or an eps that could not be applied, {"last_clock_ppm": the value applied, a 0-d tensor,
    "last_clock_ppm_packets": the estimates [F] ("auto" only)})."""
    how, half_taps = clock
    F = starts.numel()
    rows = {}
    if how == "auto":
        est = eng.clock_offset(eng.demod_frames(x, starts, want=("slope", "status"))["slope"])
        rows["last_clock_ppm_packets"] = est * 1e6
        eps = torch.nanmedian(torch.where(torch.isfinite(est), est, torch.full_like(est, float("nan"))))
        rows["last_clock_ppm"] = eps * 1e6
    else:
        rows["last_clock_ppm"] = torch.full((), how, dtype=torch.float64, device=eng.device)
        eps = rows["last_clock_ppm"] * 1e-6
    out, offsets, status = eng.resample_frames(x, starts, eps.expand(F).contiguous(), half_taps=half_taps)
    return out, offsets, status, rows


def window_stage(eng, x, starts, taper):
    """The receive window of one recording (taper = the plan's `window`, not 0), on the samples as blanking and the clock
    correction left them -> (rows, offsets: what the demodulator takes in place of (x, starts), status int32 [F]: non-zero
    for a packet that is not inside the samples, {"window_sums": per packet the two sums of Engine.window_frames' report over
    its symbols, float64 [F, 2]; `window_report` turns them into `last_window_report`})."""
    rows, offsets, status, report = eng.window_frames(x, starts, taper)
    return rows, offsets, status, {"window_sums": report.sum(dim=1)}


def window_report(plan, got):
    """`last_window_report` of a receive call from its fetched rows: None with the stage off, else the taper and per packet
    (per recording and packet for several recordings) 10 log10 of the prefix mismatch over the power it is measured against."""
    if not plan.window:
        return None
    with np.errstate(divide="ignore", invalid="ignore"):
        sums = got["window_sums"]
        return {"taper": plan.window, "mismatch_db": 10.0 * np.log10(sums[..., 0] / sums[..., 1])}


def demodulate(eng, plan, x, starts, need_eq):
    """The demodulator call of a receive call, on one recording: Hs, He, slopes, ragged flag; eq where the decode stage works
    on the equalised symbols (need_eq), eq and Hest for the plots; LLRs straight from the samples when fused.  Under
    `channel_denoising` the estimate behind all of them is the denoised one, and 'denoise_report' comes back too."""
    want = ("Hs", "He", "slope", "status") + (("Hest", "eq") if plan.plots else ("eq",) if need_eq and not plan.fused else ())
    if plan.fused:
        return eng.demod_frames_llr(x, starts, weight="csi", want=want)
    return eng.demod_frames(x, starts, want=want, denoise=plan.denoise)
