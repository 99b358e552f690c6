#!/usr/bin/env python3
"""Cost of the noise-weighted soft demapper (csrc/gf3rx_noise.hip) next to the CSI-weighted one, one JSON line.

    python tools/time_noise.py [--packets 256] [--reps 7]

Mode A2 geometry (D = 180, C = 1400, QPSK); `packets` packets of noisy equalised symbols (256 packets = 1.03 GB of eq:
far beyond the caches).  Event-timed medians after one warm-up launch of noise_estimate, soft_demap_nw and
soft_demap_csi on the same eq, the bytes each must move at least (eq read once per kernel, LLRs written once; the CSI
path writes its LLRs, then reads and rewrites them, and reads Hs / He) and the rate that makes."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd.OFDM import receiver  # noqa: E402


def ev_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    eng = receiver("A2", encoding="None")._engine()
    cfg = eng.cfg
    F, D, C, K, mu = a.packets, cfg.D, cfg.C, cfg.K, cfg.mu
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(1)
    n = F * D * C
    sign = lambda: (torch.randint(0, 2, (n,), device=dev, generator=g).double() * 2 - 1) / np.sqrt(2)
    eq = torch.complex(sign() + 0.3 * torch.randn(n, device=dev, generator=g, dtype=torch.float64),
                       sign() + 0.3 * torch.randn(n, device=dev, generator=g, dtype=torch.float64)).reshape(F * D, C)
    Hs = torch.complex(torch.randn((F, K), device=dev, generator=g, dtype=torch.float64),
                       torch.randn((F, K), device=dev, generator=g, dtype=torch.float64))
    He = Hs * 1.1
    llr = torch.empty(n * mu, dtype=torch.float32, device=dev)
    var = eng.noise_estimate(eq)
    b_eq, b_llr = n * 16, n * mu * 4
    legs = {
        "noise_estimate": (lambda: eng.noise_estimate(eq), b_eq + F * C * 8),
        "soft_demap_nw": (lambda: eng.soft_demap_nw(eq, var, out=llr), b_eq + b_llr + F * C * 8),
        "soft_demap_csi": (lambda: eng.soft_demap_csi(eq, Hs, He, out=llr), b_eq + 3 * b_llr + 2 * F * K * 16),
    }
    res = {"packets": F, "D": D, "C": C, "mu": mu, "reps": a.reps, "device": torch.cuda.get_device_name(dev)}
    for name, (fn, by) in legs.items():
        ms = ev_ms(fn, a.reps)
        res[name] = {"ms": ms, "bytes": by, "GBps": by / ms / 1e6}
    new_ms = res["noise_estimate"]["ms"] + res["soft_demap_nw"]["ms"]
    new_by = res["noise_estimate"]["bytes"] + res["soft_demap_nw"]["bytes"]
    res["noise_path_over_csi"] = {"time_ratio": new_ms / res["soft_demap_csi"]["ms"],
                                  "byte_ratio": new_by / res["soft_demap_csi"]["bytes"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
