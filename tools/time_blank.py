#!/usr/bin/env python3
"""Cost of the impulse blanking pass (csrc/gf3rx_blank.hip), one JSON line, written to profiles/blank_time.json.

    python tools/time_blank.py [--packets 256 3] [--reps 7] [--out profiles/blank_time.json]

Mode A2 geometry (S = 4320, 2P + D = 220 symbols, chirp-prefixed packets back to back), float32 samples made on the device:
Gaussian samples (what an OFDM body looks like to this pass) and the same with a 200-sample burst at 20 x the level in 60 % of
the symbols.  Event-timed medians after one warm-up launch (the scheme of tools/time_noise.py), in one process, for each
packet count: the `clone` Engine.blank_impulses makes, gf3_blank_impulses itself (its three launches, into buffers
allocated beforehand) on the clean and on the clicked stream, a `copy_` of the same bytes, and demod_frames of the same
packets (the stage that follows).  Expected from byte counts: the call reads the bodies twice and writes almost nothing,
8 B per float32 sample, as much as the clone or the copy moves.  No ratio is promised; the numbers are reported."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd import _lib  # noqa: E402
from gf3_audio_modem_amd.OFDM import receiver  # noqa: E402
from tools.time_noise import ev_ms  # noqa: E402


def one(eng, F, reps):
    cfg, dev = eng.cfg, eng.device
    M, S, Lc = cfg.M, cfg.S, cfg.chirp_length
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((F, Lc + M * S), device=dev, generator=g, dtype=torch.float32)
    off = torch.arange(F, device=dev, dtype=torch.int64) * (Lc + M * S) + Lc
    hit = torch.rand((F, M, 1), device=dev, generator=g) < 0.6
    at = torch.randint(0, S - 200, (F, M, 1), device=dev, generator=g)
    k = torch.arange(S, device=dev).reshape(1, 1, S)
    burst = hit & (k >= at) & (k < at + 200)
    clicked = x.clone()
    clicked[:, Lc:] += (burst * torch.randn((F, M, S), device=dev, generator=g, dtype=torch.float32) * 20.0).reshape(F, M * S)
    del burst
    x, clicked = x.reshape(-1), clicked.reshape(-1)
    out = x.clone()
    counts = torch.empty((F, M), dtype=torch.int32, device=dev)
    level = torch.empty((F, 2), dtype=torch.float64, device=dev)
    energy = torch.empty((F, M), dtype=torch.float64, device=dev)
    p = _lib.ptr

    def blank(src):
        eng._check(eng.lib.gf3_blank_impulses(eng._h, p(src), src.numel(), p(off), F, 4.5, 8, p(out), p(energy), p(level),
                                              p(counts), eng._stream()))

    n_body, n_all = F * M * S, x.numel()
    legs = {
        "clone": (lambda: x.clone(), 8 * n_all),
        "blank_impulses_clean": (lambda: blank(x), 8 * n_body),
        "blank_impulses_clicked": (lambda: blank(clicked), 8 * n_body),
        "copy_": (lambda: out.copy_(x), 8 * n_all),
        "demod_frames": (lambda: eng.demod_frames(x, off), 4 * n_body),
    }
    res = {"packets": F, "samples": n_all}
    for name, (fn, by) in legs.items():
        ms = ev_ms(fn, reps)
        res[name] = {"ms": ms, "bytes": by, "GBps": by / ms / 1e6}
        if name.startswith("blank"):
            res[name]["blanked_samples"] = int(counts.sum())
            res[name]["level"] = float(level[:, 1].mean())
    res["clone_plus_blank_over_copy"] = (res["clone"]["ms"] + res["blank_impulses_clicked"]["ms"]) / res["copy_"]["ms"]
    res["clone_plus_blank_over_demod"] = (res["clone"]["ms"] + res["blank_impulses_clicked"]["ms"]) / res["demod_frames"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, nargs="+", default=[256, 3])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blank_time.json"))
    a = ap.parse_args()
    eng = receiver("A2", encoding="None")._engine(np.dtype("float32"))
    cfg = eng.cfg
    res = {"S": cfg.S, "M": cfg.M, "dtype": "float32", "threshold": 4.5, "guard": 8, "reps": a.reps,
           "device": torch.cuda.get_device_name(eng.device), "compute_units": eng.n_cu,
           "runs": [one(eng, F, a.reps) for F in a.packets]}
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
