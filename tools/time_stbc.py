#!/usr/bin/env python3
"""Cost of transmit diversity (csrc/gf3rx_stbc.hip), one JSON line, written to profiles/stbc_time.json.

    python tools/time_stbc.py [--packets 64] [--reps 7] [--out profiles/stbc_time.json]

Mode A2 with 20 + 180 + 20 symbols (C = 1400, QPSK) and 64 packets; repetition scheme of tools/time_mimo.py: event-timed
medians after one warm-up launch, all in one process.  For B = 1, 2 and 4: stbc_detect beside a device copy of the bytes it
moves (B x 16 read and 8 written per cell) and beside mimo_detect at the same F, D, C and B (B x 16 read, 16 written, with
its own copy); stbc_slope beside a copy of the bytes it reads (B x 4 estimates over the fit range) -- a few hundred
kilobytes, so that row is launch latency on both sides.  Then the whole receive_stbc (wall clock, uploads included) on ONE
recording of a transmit_stbc stream.  Nothing here has a parent to be faster than: no ratio is promised, the numbers are
reported."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd.OFDM import receiver  # noqa: E402
from tools.time_noise import ev_ms  # noqa: E402


def copy_ms(nbytes, reps, dev):
    src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    return ev_ms(lambda: dst.copy_(src), reps)


def kernels(eng, F, reps):
    cfg = eng.cfg
    D, C, K, mu, NB = cfg.D, cfg.C, cfg.K, cfg.mu, cfg.N // 2 + 1
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(1)
    cn = lambda *shape: torch.complex(*torch.randn(2, *shape, device=dev, generator=g, dtype=torch.float64))
    res = {}
    n = F * D * C
    fit = min(cfg.fit_hi, K) - cfg.fit_lo
    llr = torch.empty(n * mu, dtype=torch.float32, device=dev)
    llr2 = torch.empty(n * 2 * mu, dtype=torch.float32, device=dev)
    for B in (1, 2, 4):
        Ys = [cn(F * D, NB) for _ in range(B)]
        Hs = [cn(F, 2, 2, K) for _ in range(B)]
        slopes = [1e-4 * torch.randn(F, device=dev, generator=g, dtype=torch.float64) for _ in range(B)]
        moved = n * (16 * B + 4 * mu)
        ms = ev_ms(lambda: eng.stbc_detect(Ys, Hs, slopes[0], out=llr), reps)
        res[f"stbc_detect_B{B}"] = {"ms": ms, "bytes": moved, "GBps": moved / ms / 1e6}
        cp = copy_ms(moved, reps, dev)
        res[f"device_copy_B{B}"] = {"ms": cp, "bytes": moved, "GBps": moved / cp / 1e6}
        res[f"stbc_detect_over_copy_B{B}"] = ms / cp
        moved2 = n * (16 * B + 2 * 4 * mu)
        ms2 = ev_ms(lambda: eng.mimo_detect(Ys, Hs, slopes, out=llr2), reps)
        cp2 = copy_ms(moved2, reps, dev)
        res[f"mimo_detect_B{B}"] = {"ms": ms2, "bytes": moved2, "GBps": moved2 / ms2 / 1e6}
        res[f"mimo_detect_over_copy_B{B}"] = ms2 / cp2
        res[f"stbc_over_mimo_detect_B{B}"] = ms / ms2
        by = F * B * 4 * fit * 16 + F * 8
        ms = ev_ms(lambda: eng.stbc_slope(Hs), reps)
        cp = copy_ms(by, reps, dev)
        res[f"stbc_slope_B{B}"] = {"ms": ms, "bytes": by, "copy_ms": cp, "over_copy": ms / cp}
        del Ys, Hs
    return res


def whole(rx, F, reps):
    """receive_stbc on ONE recording of F packets: the microphone hears speaker 0 and half of speaker 1, 7 samples late"""
    bits = np.random.default_rng(2).integers(0, 2, size=F * rx.packet_length * rx.data_bits_per_symbol)
    np.random.seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        tx2 = rx.transmit_stbc(bits)
    y = np.zeros(tx2.shape[1] + 600)
    y[300: 300 + tx2.shape[1]] += tx2[0]
    y[307: 307 + tx2.shape[1]] += 0.5 * tx2[1]
    del tx2
    took = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            got, _, _ = rx.receive_stbc([y])
        took.append((time.perf_counter() - t0) * 1e3)
    return {"ms": statistics.median(took[1:]), "first_call_ms": took[0], "bit_errors": int(np.sum(got != bits)), "bits": len(bits),
            "samples": len(y)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stbc_time.json"))
    a = ap.parse_args()
    rx = receiver("A2", encoding="None")
    eng = rx._engine()
    cfg = eng.cfg
    res = {"packets": a.packets, "P": cfg.P, "D": cfg.D, "C": cfg.C, "mu": cfg.mu, "reps": a.reps,
           "device": torch.cuda.get_device_name(eng.device), "compute_units": eng.n_cu}
    res.update(kernels(eng, a.packets, a.reps))
    torch.cuda.empty_cache()
    res["receive_stbc_B1"] = whole(rx, a.packets, min(a.reps, 3))
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
