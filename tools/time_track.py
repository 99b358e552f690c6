#!/usr/bin/env python3
"""Cost of the phase tracker (csrc/gf3rx_track.hip), one JSON line, written to profiles/track_time.json.

    python tools/time_track.py [--packets 256 3] [--reps 7] [--out profiles/track_time.json]

Geometry and repetition scheme of tools/time_noise.py: mode A2 (D = 180, C = 1400, QPSK), noisy equalised symbols under
a slow phase swing, event-timed medians after one warm-up launch.  Timed in one process, on the same eq, for each packet
count: track_phase out of place and in place, a device copy of the same bytes, and noise_estimate2 + soft_demap_nw2 (the
stages that follow it on the staged path).  The tracker has no parent to be faster than: no ratio is promised, the numbers
are reported.  One workgroup walks a packet's 180 symbols in sequence, so 3 packets use 3 compute units and the time per
symbol there is the length of the chain load -> two sincos per element -> butterfly -> barrier -> store, not memory."""
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


def one(eng, F, reps):
    cfg = eng.cfg
    D, C, mu = cfg.D, cfg.C, cfg.mu
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(1)
    n = F * D * C
    sign = lambda: (torch.randint(0, 2, (n,), device=dev, generator=g).double() * 2 - 1) / np.sqrt(2)
    eq = torch.complex(sign() + 0.3 * torch.randn(n, device=dev, generator=g, dtype=torch.float64),
                       sign() + 0.3 * torch.randn(n, device=dev, generator=g, dtype=torch.float64)).reshape(F, D, C)
    kap = torch.arange(C, device=dev, dtype=torch.float64) - (C - 1) / 2
    swing = torch.sin(torch.pi * (torch.arange(D, device=dev, dtype=torch.float64) + 0.5) / D) ** 2
    eq = (eq * torch.polar(torch.ones((), dtype=torch.float64, device=dev), swing[:, None] * (2.0 + 4.0 * kap / kap.max()))).reshape(F * D, C)
    out, other = torch.empty_like(eq), eq.clone()
    llr = torch.empty(n * mu, dtype=torch.float32, device=dev)
    _, phase, measured = eng.track_phase(eq, want_track=True)
    var_c, var_s = eng.noise_estimate2(eq)
    b_eq, b_llr, b_v = n * 16, n * mu * 4, F * (C + D) * 8
    legs = {
        "track_phase": (lambda: eng.track_phase(eq, out=out), 2 * b_eq),
        "track_phase_in_place": (lambda: eng.track_phase(other, out=other), 2 * b_eq),
        "device_copy": (lambda: out.copy_(eq), 2 * b_eq),
        "noise_estimate2": (lambda: eng.noise_estimate2(eq), b_eq + b_v),
        "soft_demap_nw2": (lambda: eng.soft_demap_nw2(eq, var_c, var_s, out=llr), b_eq + b_llr + b_v),
    }
    res = {"packets": F, "measured_symbols": int(measured.sum()), "symbols": F * D}
    for name, (fn, by) in legs.items():
        ms = ev_ms(fn, reps)
        res[name] = {"ms": ms, "bytes": by, "GBps": by / ms / 1e6}
    res["us_per_symbol_of_a_packet"] = 1e3 * res["track_phase"]["ms"] / (D * -(-F // eng.n_cu))
    res["over_copy"] = res["track_phase"]["ms"] / res["device_copy"]["ms"]
    res["over_noise2d_pair"] = res["track_phase"]["ms"] / (res["noise_estimate2"]["ms"] + res["soft_demap_nw2"]["ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, nargs="+", default=[256, 3])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_time.json"))
    a = ap.parse_args()
    eng = receiver("A2", encoding="None")._engine()
    cfg = eng.cfg
    res = {"D": cfg.D, "C": cfg.C, "mu": cfg.mu, "reps": a.reps, "device": torch.cuda.get_device_name(eng.device),
           "compute_units": eng.n_cu, "runs": [one(eng, F, a.reps) for F in a.packets]}
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
