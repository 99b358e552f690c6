#!/usr/bin/env python3
"""Cost of 2 x 2 spatial multiplexing (csrc/gf3rx_mimo.hip), one JSON line, written to profiles/mimo_time.json.

    python tools/time_mimo.py [--pairs 64] [--reps 7] [--out profiles/mimo_time.json]

Mode A2 with 20 + 180 + 20 symbols (C = 1400, QPSK) and 64 packet pairs; repetition scheme of tools/time_noise.py:
event-timed medians after one warm-up launch.  Timed in one process: mimo_pilots on one recording; mimo_detect at B = 2
and B = 4; beside each of those combine_branches (csi weights, LLRs only) at the same F, D, C and B -- an existing kernel
that moves comparable bytes -- and a device copy of the bytes the detector reads and writes (B x 16 per cell read, 16
written); and the whole receive_mimo (wall clock, uploads included) on two recordings of a transmit_mimo stream.
Nothing here has a parent to be faster than: no ratio is promised, the numbers are reported."""
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


def kernels(eng, F, reps):
    cfg = eng.cfg
    D, C, K, mu, NB = cfg.D, cfg.C, cfg.K, cfg.mu, cfg.N // 2 + 1
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(1)
    cn = lambda *shape: torch.complex(*torch.randn(2, *shape, device=dev, generator=g, dtype=torch.float64))
    res = {}
    # the pilot estimate: F packets back to back in one recording
    L = cfg.M * cfg.S
    x = torch.randn(F * L, device=dev, generator=g, dtype=torch.float64)
    off = torch.arange(F, dtype=torch.int64, device=dev) * L
    ms = ev_ms(lambda: eng.mimo_pilots(x, off), reps)
    by = F * (2 * cfg.P * cfg.N * 8 + 4 * K * 16)
    res["mimo_pilots"] = {"ms": ms, "bytes": by, "GBps": by / ms / 1e6}
    ms = ev_ms(lambda: eng.demod_frames(x, off, want=("Hs", "He", "slope", "status")), reps)
    res["demod_frames_for_the_slope"] = {"ms": ms}
    ms = ev_ms(lambda: eng.rfft_batch(x, (off[:, None] + (cfg.P + torch.arange(D, device=dev)) * cfg.S + cfg.CP).reshape(-1)), reps)
    res["rfft_batch_data_symbols"] = {"ms": ms}
    del x
    n = F * D * C
    llr = torch.empty(n * 2 * mu, dtype=torch.float32, device=dev)
    llr1 = torch.empty(n * mu, dtype=torch.float32, device=dev)
    for B in (2, 4):
        Ys = [cn(F * D, NB) for _ in range(B)]
        Hs = [cn(F, 2, 2, K) for _ in range(B)]
        slopes = [1e-4 * torch.randn(F, device=dev, generator=g, dtype=torch.float64) for _ in range(B)]
        moved = n * (16 * B + 16)
        ms = ev_ms(lambda: eng.mimo_detect(Ys, Hs, slopes, out=llr), reps)
        res[f"mimo_detect_B{B}"] = {"ms": ms, "bytes": moved, "GBps": moved / ms / 1e6}
        eqs = [y[:, :C].contiguous() for y in Ys]
        start, end = [h[:, 0, 0].contiguous() for h in Hs], [h[:, 1, 0].contiguous() for h in Hs]
        by = n * (16 * B + 4 * mu)
        ms = ev_ms(lambda: eng.combine_branches(eqs, Hs=start, He=end, out={"llr": llr1}, want=("llr",)), reps)
        res[f"combine_branches_B{B}"] = {"ms": ms, "bytes": by, "GBps": by / ms / 1e6}
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        ms = ev_ms(lambda: dst.copy_(src), reps)
        res[f"device_copy_B{B}"] = {"ms": ms, "bytes": moved, "GBps": moved / ms / 1e6}
        res[f"detect_over_copy_B{B}"] = res[f"mimo_detect_B{B}"]["ms"] / ms
        res[f"detect_over_combine_B{B}"] = res[f"mimo_detect_B{B}"]["ms"] / res[f"combine_branches_B{B}"]["ms"]
        del Ys, eqs, src, dst
    return res


def whole(rx, F, reps):
    """receive_mimo on two recordings of F packet pairs: microphone b hears its own speaker and half of the other, 7 samples late"""
    bits = np.random.default_rng(2).integers(0, 2, size=2 * F * rx.packet_length * rx.data_bits_per_symbol)
    np.random.seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        tx2 = rx.transmit_mimo(bits)
    rec = []
    for b in range(2):
        y = np.zeros(tx2.shape[1] + 600)
        y[300: 300 + tx2.shape[1]] += tx2[0] * (1.0 if b == 0 else 0.5)
        y[307: 307 + tx2.shape[1]] += tx2[1] * (0.5 if b == 0 else 1.0)
        rec.append(y)
    del tx2
    took = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            got, _, _ = rx.receive_mimo(rec)
        took.append((time.perf_counter() - t0) * 1e3)
    errors = int(np.sum(got != bits))
    return {"ms": statistics.median(took[1:]), "first_call_ms": took[0], "bit_errors": errors, "bits": len(bits),
            "samples_per_recording": len(rec[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mimo_time.json"))
    a = ap.parse_args()
    rx = receiver("A2", encoding="None")
    eng = rx._engine()
    cfg = eng.cfg
    res = {"pairs": a.pairs, "P": cfg.P, "D": cfg.D, "C": cfg.C, "mu": cfg.mu, "reps": a.reps,
           "device": torch.cuda.get_device_name(eng.device), "compute_units": eng.n_cu}
    res.update(kernels(eng, a.pairs, a.reps))
    torch.cuda.empty_cache()
    res["receive_mimo_B2"] = whole(rx, a.pairs, min(a.reps, 3))
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
