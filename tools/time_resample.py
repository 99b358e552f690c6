#!/usr/bin/env python3
"""Cost of the sampling-clock correction (csrc/gf3rx_resample.hip), one JSON line, written to profiles/resample_time.json.

    python tools/time_resample.py [--packets 256 3] [--reps 7] [--ppm 50] [--out profiles/resample_time.json]

The bench shape (N = 4096, CP = 512, P = 2, D = 8: S = 4608, 12 symbols, 55 296 samples per body), float32 samples made on
the device, chirp-prefixed packets back to back.  Event-timed medians after one warm-up launch (the scheme of
tools/time_noise.py), in one process, for each packet count: gf3_resample_frames itself (one launch, into buffers allocated
beforehand) at half_taps 16 and 32 with every packet at --ppm, a `copy_` of the bodies' bytes, and demod_frames of the same
packets (the stage that follows; under "auto" it also runs once before).  Expected from counts: per output 2T fp64
multiply-adds on the samples, 2T more and 2T subtractions to form the coefficients, 2T LDS reads of 8 bytes and two table
rows of 16 T bytes (from LDS where the tile's rows fit there, else from L1 / L2); 4 bytes read and 4 written per sample of HBM traffic.  No ratio is promised; the numbers
are reported."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd import _lib  # noqa: E402
from gf3_audio_modem_amd.engine import Engine, RxConfig, qpsk_table  # noqa: E402
from tools.time_noise import ev_ms  # noqa: E402


def one(eng, F, reps, ppm):
    cfg, dev = eng.cfg, eng.device
    M, S, Lc = cfg.M, cfg.S, cfg.chirp_length
    n = M * S
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((F, Lc + n), device=dev, generator=g, dtype=torch.float32).reshape(-1)
    off = torch.arange(F, device=dev, dtype=torch.int64) * (Lc + n) + Lc
    eps = torch.full((F,), ppm * 1e-6, dtype=torch.float64, device=dev)
    rows = torch.empty((F, n), dtype=torch.float32, device=dev)
    src = torch.empty((F, n), dtype=torch.float32, device=dev)
    status = torch.empty((F,), dtype=torch.int32, device=dev)
    rows_off = torch.arange(F, device=dev, dtype=torch.int64) * n
    p = _lib.ptr

    def resample(T):
        eng._check(eng.lib.gf3_resample_frames(eng._h, p(x), x.numel(), p(off), F, p(eps), T, p(rows), p(status), eng._stream()))

    legs = {
        "resample_T16": lambda: resample(16),
        "resample_T32": lambda: resample(32),
        "copy_": lambda: rows.copy_(src),
        "demod_frames": lambda: eng.demod_frames(rows, rows_off),
    }
    res = {"packets": F, "body_samples": F * n}
    for name, fn in legs.items():
        ms = ev_ms(fn, reps)
        res[name] = {"ms": ms, "Gsamples_per_s": F * n / ms / 1e6}
    assert not status.any()
    for T in (16, 32):
        taps = 2 * T
        r = res[f"resample_T{T}"]
        r["fp64_Gops_per_s"] = 3 * taps * F * n / r["ms"] / 1e6          # (one subtraction and two multiply-adds per tap)
        r["lds_read_GBps"] = 8 * taps * F * n / r["ms"] / 1e6
        r["table_read_GBps"] = 16 * taps * F * n / r["ms"] / 1e6         # (rows p and p + 1, from LDS or L1 / L2)
        r["over_demod_frames"] = r["ms"] / res["demod_frames"]["ms"]
        r["over_copy"] = r["ms"] / res["copy_"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, nargs="+", default=[256, 3])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ppm", type=float, default=50.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_time.json"))
    a = ap.parse_args()
    pts, bits = qpsk_table()
    cfg = RxConfig(N=4096, CP=512, P=2, D=8, data_bins=np.arange(100, 1500), const_points=pts, const_bits=bits,
                   known_bits=np.random.default_rng(0).integers(0, 2, size=2 * 2047).astype(np.uint8), in_dtype=torch.float32)
    eng = Engine(cfg)
    res = {"N": cfg.N, "CP": cfg.CP, "P": cfg.P, "D": cfg.D, "dtype": "float32", "ppm": a.ppm, "reps": a.reps,
           "device": torch.cuda.get_device_name(eng.device), "compute_units": eng.n_cu,
           "runs": [one(eng, F, a.reps, a.ppm) for F in a.packets]}
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
