#!/usr/bin/env python3
"""Cost of the pilot-measured joint weights (csrc/gf3rx_joint_noise.hip and the weighted instantiations of
csrc/gf3rx_mimo.hip, csrc/gf3rx_stbc.hip), one JSON line, written to profiles/joint_noise_time.json.

    python tools/time_joint_noise.py [--packets 64] [--reps 15] [--out profiles/joint_noise_time.json]

The shapes of tools/time_mimo.py and tools/time_stbc.py: mode A2 with 20 + 180 + 20 symbols (C = 1400, QPSK), 64 packets or
pairs, B = 1, 2 and 4; event-timed after one warm-up launch, all in one process.
  - mimo_pilot_noise beside mimo_pilots and demod_frames on the same samples and offsets: the estimate transforms the 2 P
    pilot symbols of a packet one by one where mimo_pilots transforms four sums; its ratio to demod_frames is what
    joint_weighting = "noise" adds to a receive call per recording.  It has no reference to be held to: reported.
  - joint_noise_weights: a few hundred kilobytes, launch latency.
  - each weighted detector beside its unweighted instantiation, the two ALTERNATING repeat by repeat, and beside a device
    copy of the bytes it must move (the unweighted call's plus 8 B per branch and carrier per workgroup).  "within_spread":
    the weighted median is no more above the unweighted median than the unweighted repeats' own max - min of this run."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd.OFDM import receiver  # noqa: E402
from tools.time_noise import ev_ms  # noqa: E402
from tools.time_stbc import copy_ms  # noqa: E402


def one_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(plain, weighted, reps):
    """Both warmed up once, then timed in turn -> ([plain ms], [weighted ms])"""
    plain()
    weighted()
    torch.cuda.synchronize()
    u, w = [], []
    for _ in range(reps):
        u.append(one_ms(plain))
        w.append(one_ms(weighted))
    return u, w


def estimate(eng, F, reps):
    cfg, dev = eng.cfg, eng.device
    L = (2 * cfg.P + cfg.D) * (cfg.N + cfg.CP)
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(F * L + 64, device=dev, generator=g, dtype=torch.float64)
    off = torch.arange(F, device=dev, dtype=torch.int64) * L + 7
    H, _ = eng.mimo_pilots(x, off)
    res = {"mimo_pilots_ms": ev_ms(lambda: eng.mimo_pilots(x, off), reps),
           "mimo_pilot_noise_ms": ev_ms(lambda: eng.mimo_pilot_noise(x, off, H), reps),
           "demod_frames_ms": ev_ms(lambda: eng.demod_frames(x, off, want=("Hs", "He", "slope", "status")), reps)}
    res["pilot_noise_over_pilots"] = res["mimo_pilot_noise_ms"] / res["mimo_pilots_ms"]
    res["pilot_noise_over_demod_frames"] = res["mimo_pilot_noise_ms"] / res["demod_frames_ms"]
    res["pilot_symbol_bytes"] = F * 2 * cfg.P * cfg.N * 8
    var, _ = eng.mimo_pilot_noise(x, off, H)
    for B in (1, 2, 4):
        res[f"joint_noise_weights_B{B}_ms"] = ev_ms(lambda: eng.joint_noise_weights([var] * B), reps)
    return res


def detectors(eng, F, reps):
    cfg, dev = eng.cfg, eng.device
    D, C, K, mu, NB = cfg.D, cfg.C, cfg.K, cfg.mu, cfg.N // 2 + 1
    g = torch.Generator(device=dev).manual_seed(1)
    cn = lambda *shape: torch.complex(*torch.randn(2, *shape, device=dev, generator=g, dtype=torch.float64))
    n = F * D * C
    out = {"mimo": torch.empty(n * 2 * mu, dtype=torch.float32, device=dev), "stbc": torch.empty(n * mu, dtype=torch.float32, device=dev)}
    res = {}
    for B in (1, 2, 4):
        Ys = [cn(F * D, NB) for _ in range(B)]
        Hs = [cn(F, 2, 2, K) for _ in range(B)]
        slopes = [1e-4 * torch.randn(F, device=dev, generator=g, dtype=torch.float64) for _ in range(B)]
        w = torch.exp(torch.randn(B, F, C, device=dev, generator=g, dtype=torch.float64))
        calls = {"mimo": lambda **kw: eng.mimo_detect(Ys, Hs, slopes, out=out["mimo"], **kw),
                 "stbc": lambda **kw: eng.stbc_detect(Ys, Hs, slopes[0], out=out["stbc"], **kw)}
        for code, call in calls.items():
            u, v = alternating(call, lambda: call(weights=w), reps)
            moved = n * 16 * B + out[code].numel() * 4
            extra = 8 * B * C * F                               # the weights, read once per workgroup: at least once per packet
            cp = copy_ms(moved + extra, reps, dev)
            mu_, mw = statistics.median(u), statistics.median(v)
            spread = max(u) - min(u)
            res[f"{code}_detect_B{B}"] = {"unweighted_ms": mu_, "weighted_ms": mw, "unweighted_spread_ms": spread,
                                          "unweighted_all_ms": u, "weighted_all_ms": v, "weighted_over_unweighted": mw / mu_,
                                          "within_spread": bool(mw - mu_ <= spread), "bytes": moved, "weight_bytes_at_least": extra,
                                          "device_copy_ms": cp, "weighted_over_copy": mw / cp}
        del Ys, Hs, w
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_noise_time.json"))
    a = ap.parse_args()
    rx = receiver("A2", encoding="None")
    eng = rx._engine()
    cfg = eng.cfg
    res = {"packets": a.packets, "P": cfg.P, "D": cfg.D, "C": cfg.C, "mu": cfg.mu, "reps": a.reps,
           "device": torch.cuda.get_device_name(eng.device), "compute_units": eng.n_cu}
    res.update(estimate(eng, a.packets, a.reps))
    torch.cuda.empty_cache()
    res.update(detectors(eng, a.packets, a.reps))
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
