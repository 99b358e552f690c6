#!/usr/bin/env python3
"""Cost of the delay-domain pilot denoiser (csrc/gf3rx_denoise.hip), one JSON line, written to profiles/denoise_time.json.

    python tools/time_denoise.py [--parent DIR] [--reps 20] [--rounds 2] [--out profiles/denoise_time.json]

Two geometries, float32 samples made on the device, chirp-prefixed packets back to back: the reference's own (N = 4096,
CP = 224, P = 20, D = 180) at F = 3, and the bench's batch shape (N = 4096, CP = 512, P = 2, D = 8) at F = 4096.  Timed are
demod_frames(split=True) -- the two-phase form as it stands -- and demod_frames(denoise=9.0), the same three launches with
denoise_kernel between the first and the second; event-timed medians of --reps calls after one warm-up (the scheme of
tools/time_noise.py), workspace allocation included in both.  Each leg runs in a process of its own; --parent DIR names a
checkout of the parent commit WITH its library built, whose two-phase form is timed side by side (--rounds alternations:
the spread between rounds is the run-to-run noise).  Expected from counts: four transforms plus P symbol reads per side
against D + 2 transforms per packet -- a few percent at D = 180, much more at D = 8.  No ratio is promised; the numbers are
reported."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEG = r"""
import json, statistics, sys
import numpy as np, torch
sys.path.insert(0, ".")
from gf3_audio_modem_amd.engine import Engine, RxConfig, qpsk_table
reps, denoise = int(sys.argv[1]), sys.argv[2] == "1"

def ev_ms(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)

pts, bits = qpsk_table()
known = np.random.default_rng(0).integers(0, 2, size=2 * 2047).astype(np.uint8)
res = []
for name, CP, P, D, F in (("reference", 224, 20, 180, 3), ("batch", 512, 2, 8, 4096)):
    eng = Engine(RxConfig(N=4096, CP=CP, P=P, D=D, data_bins=np.arange(100, 1500), const_points=pts, const_bits=bits,
                          known_bits=known, in_dtype=torch.float32))
    cfg, dev = eng.cfg, eng.device
    n, Lc = cfg.M * cfg.S, cfg.chirp_length
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((F, Lc + n), device=dev, generator=g, dtype=torch.float32).reshape(-1)
    off = torch.arange(F, device=dev, dtype=torch.int64) * (Lc + n) + Lc
    row = {"geometry": name, "CP": CP, "P": P, "D": D, "packets": F, "split_ms": ev_ms(lambda: eng.demod_frames(x, off, split=True))}
    if denoise:
        row["denoise_ms"] = ev_ms(lambda: eng.demod_frames(x, off, denoise=9.0))
        row["denoise_over_split"] = row["denoise_ms"] / row["split_ms"]
        row["applied_rows"] = int(eng.demod_frames(x, off, denoise=9.0)["denoise_report"][:, :, 4].sum().item())
    res.append(row)
    eng.close()
print("LEG " + json.dumps({"device": torch.cuda.get_device_name(0), "runs": res}))
"""


def leg(tree, reps, denoise):
    out = subprocess.run([sys.executable, "-c", LEG, str(reps), "1" if denoise else "0"], cwd=tree, capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit(f"leg in {tree} failed ({out.returncode}):\n{out.stdout}\n{out.stderr}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("LEG ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_time.json"))
    a = ap.parse_args()
    res = {"N": 4096, "dtype": "float32", "reps": a.reps, "threshold": 9.0, "rounds": []}
    for _ in range(a.rounds):
        rnd = {}
        if a.parent:
            rnd["parent"] = leg(os.path.abspath(a.parent), a.reps, False)["runs"]
        this = leg(ROOT, a.reps, True)
        rnd["this"], res["device"] = this["runs"], this["device"]
        res["rounds"].append(rnd)
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
