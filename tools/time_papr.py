#!/usr/bin/env python3
"""Transmit with tone reservation against plain transmit, one JSON line.  Records, asserts nothing.

    python tools/time_papr.py [--packets 64] [--reps 7] [--parent-lib PATH] [--out profiles/papr_time.json]

On `packets` mode-A2 packets (N = 4096, CP = 224, P = 20, D = 180, C = 1400, Ku = 647; f64 rows): tone_reserve +
tx_frames(tones) for I = 4, 16 and 64 iterations against plain tx_frames, event-timed medians of `reps` runs after one
warm-up.  The iteration runs 2 I + 1 transforms per data symbol against tx_kernel's one.  --parent-lib: a libgf3rx.so built
from the commit before the feature; its plain tx_frames is then timed in a child process of its own (GF3_LIB) at the same
packets and recorded next to this build's."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("gf3_tx_frames_ex", "gf3_tone_reserve")


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


def engine():
    from gf3_audio_modem_amd import Engine, RxConfig
    known = np.unpackbits(np.load(os.path.join(ROOT, "gf3_audio_modem_amd", "data", "known_bits.npz"))["packed"])
    return Engine(RxConfig(N=4096, CP=224, P=20, D=180, data_bins=np.arange(100, 1500), known_bits=known, in_dtype=torch.float64))


def plain_ms(eng, F, reps):
    gen = torch.Generator(device="cuda").manual_seed(7)
    payload = torch.randint(0, 256, (F, eng.bytes_per_frame), dtype=torch.uint8, device="cuda", generator=gen)
    filler = np.full(eng.cfg.K, eng.cfg.const_points[0], dtype=complex)
    return payload, filler, ev_ms(lambda: eng.tx_frames(payload, filler, out_dtype=torch.float64), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--plain-only", action="store_true", help="time plain tx_frames alone (the child process of --parent-lib)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "papr_time.json"))
    a = ap.parse_args()
    if a.plain_only:
        from gf3_audio_modem_amd import _lib
        for name in NEW:                                                 # (a library from before the feature does not export them)
            _lib._SIGS.pop(name, None)
        eng = engine()
        print(json.dumps({"plain_tx_frames_ms": plain_ms(eng, a.packets, a.reps)[2]}))
        return
    eng = engine()
    payload, filler, plain = plain_ms(eng, a.packets, a.reps)
    res = {"reps": a.reps, "device": torch.cuda.get_device_name(0), "packets": a.packets, "symbols": a.packets * eng.cfg.D,
           "N": 4096, "D": 180, "C": 1400, "Ku": eng.cfg.K - eng.cfg.C, "plain_tx_frames_ms": plain}
    if a.parent_lib:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--packets", str(a.packets), "--reps", str(a.reps)],
                             env={**os.environ, "GF3_LIB": os.path.abspath(a.parent_lib)}, capture_output=True, text=True, check=True, timeout=300)
        res["parent_plain_tx_frames_ms"] = json.loads(out.stdout.strip().splitlines()[-1])["plain_tx_frames_ms"]
    base = res.get("parent_plain_tx_frames_ms", plain)
    for iters in (4, 16, 64):
        def both():
            tones, _ = eng.tone_reserve(payload, iterations=iters)
            eng.tx_frames(payload, filler, out_dtype=torch.float64, tones=tones)
        ms_r = ev_ms(lambda: eng.tone_reserve(payload, iterations=iters), a.reps)
        ms = ev_ms(both, a.reps)
        rep = eng.tone_reserve(payload, iterations=iters)[1]
        res[f"I{iters}"] = {"tone_reserve_ms": ms_r, "tone_reserve_plus_tx_frames_ms": ms, "ratio_to_plain": ms / base,
                            "transforms_per_symbol": 2 * iters + 1, "mean_best_index": float(rep[..., 2].mean()),
                            "mean_peak_zero_filler": float(rep[..., 0].mean()), "mean_best_peak": float(rep[..., 1].mean())}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
