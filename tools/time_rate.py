#!/usr/bin/env python3
"""Cost of the whole-stream rate conversion (gf3_resample_stream, csrc/gf3rx_resample.hip), one JSON line, written to
profiles/rate_time.json.

    python tools/time_rate.py [--samples 3000000] [--reps 7] [--out profiles/rate_time.json]

A recording of --samples float32 samples made on the device, taken at 44.1 kHz (r = 147/160: the up path, 2T taps per
output) and at 96 kHz (r = 2: the down path, 4T taps per output, each with its own two table rows), converted to 48 kHz on
the standard geometry's float32 engine (N = 4096, CP = 224, carriers 100 .. 1499).  Event-timed medians after one warm-up
launch (the scheme of tools/time_noise.py), in one process: gf3_resample_stream itself (one launch, into a buffer allocated
beforehand) at half_taps 16 and 32, a `copy_` of the input's bytes and one of the output's, and sync_stream of the result
(the stage that follows).  Expected from counts: per output W = 2T (up) or 2 ceil(T r) (down) fp64 multiply-adds on the
samples, W more and W subtractions to form the coefficients, W LDS reads of 8 bytes and two table rows (up: 16 T bytes
each; down: two 8-byte words per tap) from L1 / L2; on the down path about ten more fp64 and integer operations per tap
find the row and the column.  4 bytes read per input sample and 4 written per output of HBM traffic.  No ratio is promised;
the numbers are reported."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd import _lib  # noqa: E402
from gf3_audio_modem_amd.engine import Engine, RxConfig, qpsk_table  # noqa: E402
from tools.time_noise import ev_ms  # noqa: E402


def one(eng, n_in, rate, reps):
    dev = eng.device
    r = rate / 48000.0
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((n_in,), device=dev, generator=g, dtype=torch.float32)
    n_out = eng.stream_outputs(n_in, r, 32, final=True)
    y = torch.empty((n_out,), dtype=torch.float32, device=dev)
    x2, y2 = torch.empty_like(x), torch.empty_like(y)
    p = _lib.ptr

    def convert(T):
        eng._check(eng.lib.gf3_resample_stream(eng._h, p(x), _lib.DT_F32, n_in, 0, r, T, 0, n_out, p(y), eng._stream()))

    legs = {
        "convert_T16": lambda: convert(16),
        "convert_T32": lambda: convert(32),
        "copy_input": lambda: x2.copy_(x),
        "copy_output": lambda: y2.copy_(y),
        "sync_stream": lambda: eng.sync_stream(y),
    }
    res = {"input_rate": rate, "r": r, "input_samples": n_in, "output_samples": n_out}
    for name, fn in legs.items():
        ms = ev_ms(fn, reps)
        res[name] = {"ms": ms}
    for T in (16, 32):
        taps = 2 * (int(math.ceil(T * r)) if r > 1.0 else T)
        c = res[f"convert_T{T}"]
        c["taps"] = taps
        c["Msamples_in_per_s"] = n_in / c["ms"] / 1e3
        c["fp64_Gops_per_s"] = 3 * taps * n_out / c["ms"] / 1e6          # (one subtraction and two multiply-adds per tap)
        c["over_copy_input"] = c["ms"] / res["copy_input"]["ms"]
        c["over_sync_stream"] = c["ms"] / res["sync_stream"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3000000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_time.json"))
    a = ap.parse_args()
    pts, bits = qpsk_table()
    cfg = RxConfig(N=4096, CP=224, P=20, D=180, data_bins=np.arange(100, 1500), const_points=pts, const_bits=bits,
                   known_bits=np.random.default_rng(0).integers(0, 2, size=2 * 2047).astype(np.uint8), in_dtype=torch.float32)
    eng = Engine(cfg)
    res = {"N": cfg.N, "CP": cfg.CP, "dtype": "float32", "reps": a.reps, "device": torch.cuda.get_device_name(eng.device),
           "compute_units": eng.n_cu, "runs": [one(eng, a.samples, rate, a.reps) for rate in (44100.0, 96000.0)]}
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
