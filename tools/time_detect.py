#!/usr/bin/env python3
"""Cost of the self-normalised chirp detection (csrc/gf3rx_detect.hip) against the reference's rule on the same stream, one
JSON line, written to profiles/detect_time.json.

    python tools/time_detect.py [--reps 20] [--rounds 2] [--out profiles/detect_time.json]

The reference's geometry (N = 4096, CP = 224, P = 20, D = 180: Lc = 21600, one chirp per 972 000 samples), float32 samples
made on the device: noise at a quarter of the chirp's amplitude with a chirp at the head of every packet, at 3 M samples (the
project's real recording) and at 2^24 (the largest piece the summation is specified for).  Timed are
Engine.sync_stream(mode=1) -- the all-fp64 overlap-save and the reference's rule, which is also the parent's code -- and
Engine.detect_stream, which runs the same overlap-save and adds one pass over the samples for the block totals, two passes
of det_rho_kernel (the largest window energy, then rho and the count) and the decision; event-timed medians of --reps calls
after one warm-up (the scheme of tools/time_noise.py), allocation of workspace and outputs included in both, the two
alternating in --rounds rounds (their spread is the run-to-run noise).  The per-kernel split is a profiler's to give
(rocprofv3 --kernel-trace --stats on one call); no ratio is promised, the numbers are reported."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=[3_000_000, 1 << 24])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_time.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from gf3_audio_modem_amd.engine import Engine, RxConfig, qpsk_table
    if not torch.cuda.is_available():
        raise SystemExit("time_detect.py measures on the GPU; none is visible")

    def ev_ms(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record(); t1.synchronize()
            out.append(t0.elapsed_time(t1))
        return statistics.median(out)

    pts, bits = qpsk_table()
    known = np.random.default_rng(0).integers(0, 2, size=2 * 2047).astype(np.uint8)
    eng = Engine(RxConfig(N=4096, CP=224, P=20, D=180, data_bins=np.arange(100, 1500), const_points=pts, const_bits=bits,
                          known_bits=known, in_dtype=torch.float32))
    cfg, dev = eng.cfg, eng.device
    chirp = torch.from_numpy(eng.chirp_replica()).to(dev, torch.float32)
    res = {"N": 4096, "dtype": "float32", "reps": a.reps, "threshold": 0.3, "device": torch.cuda.get_device_name(0), "runs": []}
    for n in a.sizes:
        g = torch.Generator(device=dev).manual_seed(1)
        x = 0.05 * torch.randn((n,), device=dev, generator=g, dtype=torch.float32)
        starts = list(range(1000, n - 2 * cfg.chirp_length, cfg.frame_len))
        for s in starts:
            x[s: s + cfg.chirp_length] += chirp
        want = torch.tensor(starts, device=dev) + cfg.chirp_length - 2
        row = {"samples": n, "chirps": len(starts), "rounds": []}
        for _ in range(a.rounds):
            rnd = {"sync_stream_fp64_ms": ev_ms(lambda: eng.sync_stream(x, mode=1)), "detect_stream_ms": ev_ms(lambda: eng.detect_stream(x))}
            rnd["detect_over_sync"] = rnd["detect_stream_ms"] / rnd["sync_stream_fp64_ms"]
            row["rounds"].append(rnd)
        row["same_detections"] = bool(torch.equal(eng.detect_stream(x), want))
        res["runs"].append(row)
    eng.close()
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
