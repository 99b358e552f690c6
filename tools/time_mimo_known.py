#!/usr/bin/env python3
"""Cost of the known-bit joint detector (gf3_mimo_detect_known, csrc/gf3rx_mimo.hip) next to gf3_mimo_detect, one JSON
line, written to profiles/mimo_known_time.json.

    python tools/time_mimo_known.py [--pairs 64] [--reps 7] [--out profiles/mimo_known_time.json]

Mode A2 with 20 + 180 + 20 symbols (C = 1400, QPSK) and 64 packet pairs, B = 2 and B = 4, random spectra, estimates and
slopes as tools/time_mimo.py makes them.  Three states of the mask: nothing known, stream 0 wholly known, a random half of
the codeword-sized runs of 1536 bits known.  Timed in one process on the same inputs, one warm-up round and then `reps`
rounds that ALTERNATE the legs -- mimo_detect, the three mask states, a device copy of the bytes the new call must move
(mimo_detect's B x 16 read + 16 written per cell, plus 8 plane bytes per cell) --, each launch between two device events;
the median, the least and the largest of each leg are kept.  `known_over_detect_*` is the ratio of medians to mimo_detect
in this same run -- the comparison against unchanged code --, `known_over_copy_*` the ratio to the copy.  No threshold
is fixed in advance; `detect_spread` = (largest - least) / median of mimo_detect's own rounds is what a difference has to
exceed to mean anything.  The all-unknown output is also compared with mimo_detect's, byte for byte."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd.OFDM import receiver  # noqa: E402

RUN = 1536


def rounds(legs, reps):
    """{name: fn} -> {name: [ms per round]}: one untimed round, then `reps` rounds, the legs one after the other in each"""
    took = {name: [] for name in legs}
    for r in range(reps + 1):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r:
                took[name].append(a.elapsed_time(b))
    return took


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mimo_known_time.json"))
    a = ap.parse_args()
    eng = receiver("A2", encoding="None")._engine()
    cfg = eng.cfg
    F, D, C, K, mu, NB = a.pairs, cfg.D, cfg.C, cfg.K, cfg.mu, cfg.N // 2 + 1
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(1)
    cn = lambda *shape: torch.complex(*torch.randn(2, *shape, device=dev, generator=g, dtype=torch.float64))
    cells = F * D * C
    n = cells * 2 * mu
    res = {"pairs": F, "P": cfg.P, "D": D, "C": C, "mu": mu, "reps": a.reps, "device": torch.cuda.get_device_name(dev),
           "compute_units": eng.n_cu}
    bits = torch.randint(0, 2, (n,), device=dev, generator=g, dtype=torch.uint8)
    known = {"none": torch.zeros(n, dtype=torch.uint8, device=dev)}
    known["stream0"] = torch.zeros((F, 2, D * C * mu), dtype=torch.uint8, device=dev)
    known["stream0"][:, 0] = 1
    known["stream0"] = known["stream0"].reshape(-1)
    runs = (torch.rand(n // RUN + 1, device=dev, generator=g) < 0.5).to(torch.uint8)
    known["half"] = runs.repeat_interleave(RUN)[:n].contiguous()
    res["known_fraction"] = {k: float(v.float().mean()) for k, v in known.items()}
    out_d = torch.empty(n, dtype=torch.float32, device=dev)
    out_k = torch.empty(n, dtype=torch.float32, device=dev)
    for B in (2, 4):
        Ys = [cn(F * D, NB) for _ in range(B)]
        Hs = [cn(F, 2, 2, K) for _ in range(B)]
        slopes = [1e-4 * torch.randn(F, device=dev, generator=g, dtype=torch.float64) for _ in range(B)]
        moved = cells * (16 * B + 16 + 8)
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        legs = {"mimo_detect": lambda: eng.mimo_detect(Ys, Hs, slopes, out=out_d)}
        for state, k in known.items():
            legs[f"known_{state}"] = lambda k=k: eng.mimo_detect_known(Ys, Hs, slopes, bits, k, out=out_k)
        legs["device_copy"] = lambda: dst.copy_(src)
        took = rounds(legs, a.reps)
        med = {name: statistics.median(v) for name, v in took.items()}
        for name, v in took.items():
            by = cells * (16 * B + 16) if name == "mimo_detect" else moved
            res[f"{name}_B{B}"] = {"ms": med[name], "min_ms": min(v), "max_ms": max(v), "bytes": by, "GBps": by / med[name] / 1e6}
        res[f"detect_spread_B{B}"] = (max(took["mimo_detect"]) - min(took["mimo_detect"])) / med["mimo_detect"]
        for state in known:
            res[f"known_over_detect_{state}_B{B}"] = med[f"known_{state}"] / med["mimo_detect"]
            res[f"known_over_copy_{state}_B{B}"] = med[f"known_{state}"] / med["device_copy"]
        eng.mimo_detect(Ys, Hs, slopes, out=out_d)
        eng.mimo_detect_known(Ys, Hs, slopes, bits, known["none"], out=out_k)
        res[f"none_is_mimo_detect_bytes_B{B}"] = bool(torch.equal(out_d.view(torch.int32), out_k.view(torch.int32)))
        del Ys, src, dst
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
