#!/usr/bin/env python3
"""Cost of the diversity combiner (csrc/gf3rx_combine.hip), one JSON line, written to profiles/diversity_time.json.

    python tools/time_diversity.py [--packets 256] [--branches 2 4] [--reps 7] [--out profiles/diversity_time.json]

Geometry and repetition scheme of tools/time_noise.py: mode A2 (D = 180, C = 1400, QPSK), noisy equalised symbols,
event-timed medians after one warm-up launch.  Timed in one process for each branch count B: combine_branches with all
three outputs under the csi weights and under the noise weights, the B noise_estimate calls the noise weights need first,
and a device copy that moves the same number of bytes as the combiner (B x 16 read, 16 + 8 + 4 mu written per symbol).
The combiner has no parent to be faster than: no ratio is promised, the numbers are reported."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd.OFDM import receiver  # noqa: E402
from tools.time_noise import ev_ms  # noqa: E402


def one(eng, F, B, reps):
    cfg = eng.cfg
    D, C, K, mu = cfg.D, cfg.C, cfg.K, cfg.mu
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(B)
    n = F * D * C
    sign = (torch.randint(0, 2, (2, n), device=dev, generator=g).double() * 2 - 1) / np.sqrt(2)
    eqs, Hs, He = [], [], []
    for b in range(B):
        noise = (0.1 + 0.1 * b) * torch.randn(2, n, device=dev, generator=g, dtype=torch.float64)
        eqs.append(torch.complex(sign[0] + noise[0], sign[1] + noise[1]).reshape(F * D, C))
        Hs.append(torch.complex(*torch.randn(2, F, K, device=dev, generator=g, dtype=torch.float64)))
        He.append(torch.complex(*torch.randn(2, F, K, device=dev, generator=g, dtype=torch.float64)))
    var = [eng.noise_estimate(e) for e in eqs]
    want = ("eq", "w", "llr")
    out = {"eq": torch.empty_like(eqs[0]), "w": torch.empty((F * D, C), dtype=torch.float64, device=dev),
           "llr": torch.empty(n * mu, dtype=torch.float32, device=dev)}
    moved = n * (16 * B + 16 + 8 + 4 * mu)
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def estimates():
        for e in eqs:
            eng.noise_estimate(e)
    legs = {
        "combine_csi": (lambda: eng.combine_branches(eqs, Hs=Hs, He=He, out=out, want=want), moved + 2 * B * F * K * 16),
        "combine_noise": (lambda: eng.combine_branches(eqs, var=var, out=out, want=want), moved + B * F * C * 8),
        "combine_noise_llr_only": (lambda: eng.combine_branches(eqs, var=var, out={"llr": out["llr"]}, want=("llr",)),
                                   n * (16 * B + 4 * mu) + B * F * C * 8),
        "noise_estimates": (estimates, B * (n * 16 + F * C * 8)),
        "device_copy": (lambda: dst.copy_(src), moved),
    }
    res = {"packets": F, "branches": B}
    for name, (fn, by) in legs.items():
        ms = ev_ms(fn, reps)
        res[name] = {"ms": ms, "bytes": by, "GBps": by / ms / 1e6}
    res["csi_over_copy"] = res["combine_csi"]["ms"] / res["device_copy"]["ms"]
    res["noise_over_copy"] = res["combine_noise"]["ms"] / res["device_copy"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=256)
    ap.add_argument("--branches", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diversity_time.json"))
    a = ap.parse_args()
    eng = receiver("A2", encoding="None")._engine()
    cfg = eng.cfg
    res = {"D": cfg.D, "C": cfg.C, "mu": cfg.mu, "reps": a.reps, "device": torch.cuda.get_device_name(eng.device),
           "compute_units": eng.n_cu, "runs": [one(eng, a.packets, B, a.reps) for B in a.branches]}
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
