#!/usr/bin/env python3
"""Cost of the loaded noise pair (csrc/gf3rx_loading.hip) next to the uniform kernels it generalises, one JSON line
(also written to profiles/loading_time.json).

    python tools/time_loading.py [--packets 256] [--reps 7]

Mode A2 geometry (D = 180, C = 1400); `packets` packets of noisy equalised symbols (256 packets = 1.03 GB of eq: far
beyond the caches).  Event-timed medians after one warm-up launch of noise_estimate_loaded, soft_demap_loaded(var) and
soft_demap_loaded(Hs, He) on five loadings: uniform 2 / 4 / 6, a smooth ramp (four long runs: 6, 4, 2, 0) and the worst
case, 0 / 2 / 4 / 6 interleaved carrier by carrier (every wave takes every branch).  Per leg: milliseconds, the bytes
that must move at least (16 B read per carrier-symbol, 4 order B written) and the rate that makes.  The yardstick
beside each uniform loading is the parent's unchanged code: noise_estimate, soft_demap_nw and soft_demap_csi on a
context built with square_qam_table(m), same symbols, same byte count (the staged CSI pair moves more than that: it
writes its LLRs, reads and rewrites them)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd import Engine, RxConfig, square_qam_table  # noqa: E402
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


def loadings(C):
    q = C // 4
    ramp = np.concatenate([np.full(q, 6), np.full(q, 4), np.full(q, 2), np.zeros(C - 3 * q)]).astype(np.uint8)
    return {"uniform2": np.full(C, 2, np.uint8), "uniform4": np.full(C, 4, np.uint8), "uniform6": np.full(C, 6, np.uint8),
            "ramp": ramp, "interleaved": np.resize([0, 2, 4, 6], C).astype(np.uint8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    rx = receiver("A2", encoding="None")
    eng = rx._engine()
    cfg = eng.cfg
    F, D, C, K = a.packets, cfg.D, cfg.C, cfg.K
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(1)
    n = F * D * C
    sign = lambda: (torch.randint(0, 2, (n,), device=dev, generator=g).double() * 2 - 1) / np.sqrt(2)
    eq = torch.complex(sign() + 0.3 * torch.randn(n, device=dev, generator=g, dtype=torch.float64),
                       sign() + 0.3 * torch.randn(n, device=dev, generator=g, dtype=torch.float64)).reshape(F * D, C)
    Hs = torch.complex(torch.randn((F, K), device=dev, generator=g, dtype=torch.float64),
                       torch.randn((F, K), device=dev, generator=g, dtype=torch.float64))
    He = Hs * 1.1
    llr = torch.empty(n * 6, dtype=torch.float32, device=dev)
    res = {"packets": F, "D": D, "C": C, "reps": a.reps, "device": torch.cuda.get_device_name(dev), "loadings": {}}

    def timed(fn, by):
        ms = ev_ms(fn, a.reps)
        return {"ms": ms, "bytes": by, "GBps": by / ms / 1e6}
    for name, order in loadings(C).items():
        ld = eng.loading(order)
        out = llr[: F * D * ld.bits]
        var = eng.noise_estimate_loaded(eq, ld)
        b_eq, b_llr = n * 16, F * D * ld.bits * 4
        legs = {"noise_estimate_loaded": timed(lambda: eng.noise_estimate_loaded(eq, ld), b_eq),
                "soft_demap_loaded_var": timed(lambda: eng.soft_demap_loaded(eq, ld, var=var, out=out), b_eq + b_llr),
                "soft_demap_loaded_csi": timed(lambda: eng.soft_demap_loaded(eq, ld, Hs=Hs, He=He, out=out), b_eq + b_llr)}
        if name.startswith("uniform"):
            m = int(order[0])
            pts, bits = square_qam_table(m)
            par = Engine(RxConfig(N=cfg.N, CP=cfg.CP, P=cfg.P, D=cfg.D, data_bins=cfg.data_bins, const_points=pts, const_bits=bits,
                                  known_bits=np.resize(np.asarray(cfg.known_bits), cfg.K * m), Lc=cfg.Lc), device=dev)
            pvar = par.noise_estimate(eq)
            legs["parent_noise_estimate"] = timed(lambda: par.noise_estimate(eq), b_eq)
            legs["parent_soft_demap_nw"] = timed(lambda: par.soft_demap_nw(eq, pvar, out=out), b_eq + b_llr)
            legs["parent_soft_demap_csi"] = timed(lambda: par.soft_demap_csi(eq, Hs, He, out=out), b_eq + b_llr)
            par.close()
        res["loadings"][name] = {"bits_per_symbol": ld.bits, **legs}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "loading_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
