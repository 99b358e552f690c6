#!/usr/bin/env python3
"""Cost of the receive window (csrc/gf3rx_window.hip), one JSON line, written to profiles/window_time.json.

    python tools/time_window.py [--reps 9] [--out profiles/window_time.json]

Two shapes, float32 samples made on the device, chirp-prefixed packets back to back at odd sample offsets (what a sync
returns): mode A2 (N = 4096, CP = 224, P = 20, D = 180: 220 symbols of 4320 samples per body) at 64 packets, and mode C2
(CP = 1184: 5280 samples per symbol) at 3 packets; each with a ramp of L = 128 samples and of L = CP.  Per shape, in one
process, the legs are timed in turn, round after round, so that a drift of the machine falls on all of them alike:

    window_frames   gf3_window_frames itself (one launch, into buffers allocated beforehand)
    copy_           a device copy of the bytes the stage must move (M S samples read and M S written per packet)
    resample_frames gf3_resample_frames at the same shape (half_taps 16, 50 ppm): the neighbouring stage
    demod_frames    the demodulator on the same samples: the stage that follows

A leg's time is the median over the rounds of an event-timed window holding enough back-to-back calls to last about 20 ms
(a single call of the small shape is a few microseconds of work); the smallest and largest round are kept too.  Bytes per
call from the shape: window_frames reads M S + L M samples and L M ramp values (8 bytes each) and writes M S samples per
packet.  No ratio is promised; the numbers are reported."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd import _lib  # noqa: E402
from gf3_audio_modem_amd.engine import Engine, RxConfig, qpsk_table  # noqa: E402

SHAPES = {"A2": dict(CP=224, packets=64), "C2": dict(CP=1184, packets=3)}
WINDOW_MS = 20.0


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def one(mode, reps):
    pts, bits = qpsk_table()
    CP, F = SHAPES[mode]["CP"], SHAPES[mode]["packets"]
    cfg = RxConfig(N=4096, CP=CP, P=20, D=180, data_bins=np.arange(100, 1500), const_points=pts, const_bits=bits,
                   known_bits=np.random.default_rng(0).integers(0, 2, size=2 * 2047).astype(np.uint8), in_dtype=torch.float32)
    eng = Engine(cfg)
    dev = eng.device
    M, S, Lc = cfg.M, cfg.S, cfg.chirp_length
    n = M * S
    stride = Lc + n + 1                                         # (odd: the bodies start at every offset within 16 bytes)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((F * stride,), device=dev, generator=g, dtype=torch.float32)
    off = torch.arange(F, device=dev, dtype=torch.int64) * stride + Lc
    eps = torch.full((F,), 50e-6, dtype=torch.float64, device=dev)
    rows = torch.empty((F, n), dtype=torch.float32, device=dev)
    src = torch.randn((F, n), device=dev, generator=g, dtype=torch.float32)
    status = torch.empty((F,), dtype=torch.int32, device=dev)
    report = torch.empty((F, M, 2), dtype=torch.float64, device=dev)
    rows_off = torch.arange(F, device=dev, dtype=torch.int64) * n
    ramps = {L: torch.from_numpy(Engine.window_ramp(L)).to(dev) for L in (128, CP)}
    p = _lib.ptr

    def window(L):
        eng._check(eng.lib.gf3_window_frames(eng._h, p(x), x.numel(), p(off), F, p(ramps[L]), L, p(rows), p(report), p(status),
                                             eng._stream()))

    def resample():
        eng._check(eng.lib.gf3_resample_frames(eng._h, p(x), x.numel(), p(off), F, p(eps), 16, p(rows), p(status), eng._stream()))

    legs = {"window_frames_L128": lambda: window(128), f"window_frames_L{CP}": lambda: window(CP), "copy_": lambda: rows.copy_(src),
            "resample_frames": resample, "demod_frames": lambda: eng.demod_frames(x, off)}
    inner = {}
    for name, fn in legs.items():                               # warm-up, and how many calls fill the window
        fn()
        torch.cuda.synchronize()
        inner[name] = max(1, min(2000, math.ceil(WINDOW_MS / max(timed(fn, 3), 1e-4))))
    rounds = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            rounds[name].append(timed(fn, inner[name]))
    assert not status.any()
    res = {"mode": mode, "CP": CP, "packets": F, "symbols": M, "body_samples": F * n, "compute_units": eng.n_cu,
           "workgroups": (M + _run(eng, F, M) - 1) // _run(eng, F, M) * F}
    for name, ms in rounds.items():
        med = statistics.median(ms)
        res[name] = {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "calls_per_window": inner[name],
                     "Gsamples_per_s": F * n / med / 1e6}
    for L in (128, CP):
        r = res[f"window_frames_L{L}"]
        moved = F * (4 * (2 * n + L * M) + 8 * L * M)
        r["bytes"] = moved
        r["GBps"] = moved / r["ms"] / 1e6
        for other in ("copy_", "resample_frames", "demod_frames"):
            r["over_" + other.rstrip("_")] = r["ms"] / res[other]["ms"]
    res["copy_"]["GBps"] = 8 * F * n / res["copy_"]["ms"] / 1e6
    return res


def _run(eng, F, M):
    """Symbols per workgroup, as gf3_window_frames sizes them (symbols_per_group, csrc/gf3rx_host.h)"""
    nchunk = min(max((8 * eng.n_cu + F - 1) // F, 1), M)
    return (M + nchunk - 1) // nchunk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_window.py measures on the GPU; none is visible")
    res = {"N": 4096, "P": 20, "D": 180, "dtype": "float32", "reps": a.reps, "window_ms": WINDOW_MS,
           "device": torch.cuda.get_device_name(0), "runs": [one(mode, a.reps) for mode in SHAPES]}
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
