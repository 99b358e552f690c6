#!/usr/bin/env python3
"""Cost of the impulse-noise pair (csrc/gf3rx_noise.hip: carrier x symbol estimate and demapper, packet interleaver) next
to the per-carrier pair it extends, one JSON line.

    python tools/time_impulse.py [--packets 256] [--reps 7]

Geometry and repetition scheme of tools/time_noise.py: mode A2 (D = 180, C = 1400, QPSK), `packets` packets of noisy
equalised symbols (256 packets = 1.03 GB of eq), event-timed medians after one warm-up launch.  Timed in one process, on
the same eq: noise_estimate + soft_demap_nw (the yardstick), noise_estimate2, soft_demap_nw2 without and with
`deinterleave`, and the bare gf3_interleave on float32 LLRs (what a de-interleave as a second kernel costs)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    eng = receiver("A2", encoding="None")._engine()
    cfg = eng.cfg
    F, D, C, mu = a.packets, cfg.D, cfg.C, cfg.mu
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(1)
    n = F * D * C
    sign = lambda: (torch.randint(0, 2, (n,), device=dev, generator=g).double() * 2 - 1) / np.sqrt(2)
    eq = torch.complex(sign() + 0.3 * torch.randn(n, device=dev, generator=g, dtype=torch.float64),
                       sign() + 0.3 * torch.randn(n, device=dev, generator=g, dtype=torch.float64)).reshape(F * D, C)
    llr = torch.empty(n * mu, dtype=torch.float32, device=dev)
    var = eng.noise_estimate(eq)
    var_c, var_s = eng.noise_estimate2(eq)
    assert torch.equal(var, var_c)
    b_eq, b_llr, b_v = n * 16, n * mu * 4, F * (C + D) * 8
    legs = {
        "noise_estimate": (lambda: eng.noise_estimate(eq), b_eq + F * C * 8),
        "soft_demap_nw": (lambda: eng.soft_demap_nw(eq, var, out=llr), b_eq + b_llr + F * C * 8),
        "noise_estimate2": (lambda: eng.noise_estimate2(eq), b_eq + b_v),
        "soft_demap_nw2": (lambda: eng.soft_demap_nw2(eq, var_c, var_s, out=llr), b_eq + b_llr + b_v),
        "soft_demap_nw2_deinterleave": (lambda: eng.soft_demap_nw2(eq, var_c, var_s, deinterleave=True, out=llr), b_eq + b_llr + b_v),
        "interleave_f32_inverse": (lambda: eng.interleave(llr, inverse=True), 2 * b_llr),
        "interleave_f32_forward": (lambda: eng.interleave(llr), 2 * b_llr),
    }
    res = {"packets": F, "D": D, "C": C, "mu": mu, "reps": a.reps, "device": torch.cuda.get_device_name(dev)}
    for name, (fn, by) in legs.items():
        ms = ev_ms(fn, a.reps)
        res[name] = {"ms": ms, "bytes": by, "GBps": by / ms / 1e6}
    t = lambda k: res[k]["ms"]
    by = lambda k: res[k]["bytes"]
    parent = t("noise_estimate") + t("soft_demap_nw")
    res["over_parent_pair"] = {
        "parent_ms": parent,
        "byte_ratio": (by("noise_estimate2") + by("soft_demap_nw2")) / (by("noise_estimate") + by("soft_demap_nw")),
        "time_ratio": (t("noise_estimate2") + t("soft_demap_nw2")) / parent,
        "time_ratio_deinterleaved": (t("noise_estimate2") + t("soft_demap_nw2_deinterleave")) / parent,
        "time_ratio_deinterleaved_by_second_kernel": (t("noise_estimate2") + t("soft_demap_nw2") + t("interleave_f32_inverse")) / parent,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
