#!/usr/bin/env python3
"""Host-side cost of the receive façade, one JSON line, written to profiles/receive_refactor_time.json.

    python tools/time_receive.py --parent DIR [--reps 20] [--rounds 3] [--out profiles/receive_refactor_time.json]

Three calls, each timed by wall clock from a host array in to bits on the host out (the call's own synchronisation ends it),
median of --reps calls after 3 warm-up calls, on one receiver per call kind:
  fst        receiver("A2", "XOR").receive() on the g6_realrec recording -- what bench.py's Final System Test leg times
  coded      a "QCLDPC-1/2" receive() under llr_weighting = "noise" on the three-packet signal of
             tests/test_receive_pipeline_gpu.py (no_pilots = 2, packet_length = 4, its case "qc_noise2d_il" without the
             interleaver and with "noise")
  diversity  a B = 2 receive_diversity() on that test's two-recording "XOR" signal
Each leg runs in a process of its own; --parent DIR names a checkout of the parent commit WITH its library built (the same
library: this change touches no kernel).  The legs alternate, parent then this tree, --rounds times.  Criterion, per call:
the median of this tree's rounds is at most the median of the parent's rounds plus the spread (max - min) of the parent's own
rounds -- the only noise figure this comparison has.  Exit status 1 where it is missed."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("fst", "coded", "diversity")

LEG = r"""
import contextlib, io, json, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, ".")
sys.path.append(sys.argv[2])                                    # (the signals: this tree's test module, in both legs)
import test_receive_pipeline_gpu as T
from gf3_audio_modem_amd.OFDM import receiver
reps, warm = int(sys.argv[1]), 3

def median_ms(fn):
    out = []
    with contextlib.redirect_stdout(io.StringIO()):
        for i in range(warm + reps):
            t = time.perf_counter()
            fn()
            if i >= warm:
                out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)

wav = np.load(sys.argv[2] + "/golden/g6_realrec.npz")["wav_u8"]
fst = receiver(mode="A2", encoding="XOR")
T.CASES["timed_coded"] = ("receive", 1, T.QC, {"llr_weighting": "noise"}, 14.0, False)
one = T.signals("timed_coded")[2]
coded = T.configured(receiver, T.QC, {"llr_weighting": "noise"})
two = T.signals("div2_xor")[2]
div = T.configured(receiver, "XOR", {})
res = {"fst": median_ms(lambda: fst.receive(wav)), "coded": median_ms(lambda: coded.receive(one[0])),
       "diversity": median_ms(lambda: div.receive_diversity(two))}
print("LEG " + json.dumps({"device": torch.cuda.get_device_name(0), "ms": res}))
"""


def leg(tree, reps):
    out = subprocess.run([sys.executable, "-c", LEG, str(reps), os.path.join(ROOT, "tests")], cwd=tree, capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit(f"leg in {tree} failed ({out.returncode}):\n{out.stdout}\n{out.stderr}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("LEG ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="checkout of the parent commit with its library built")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "receive_refactor_time.json"))
    a = ap.parse_args()
    rounds = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for name, tree in (("parent", os.path.abspath(a.parent)), ("this", ROOT)):
            got = leg(tree, a.reps)
            rounds[name].append(got["ms"])
    res = {"timing": f"wall clock, ms per call, median of {a.reps} calls after 3; {a.rounds} alternating rounds", "device": got["device"],
           "rounds": rounds, "calls": {}}
    for call in CALLS:
        parent, this = [r[call] for r in rounds["parent"]], [r[call] for r in rounds["this"]]
        row = {"parent_median_ms": statistics.median(parent), "this_median_ms": statistics.median(this),
               "parent_spread_ms": max(parent) - min(parent)}
        row["no_regression"] = row["this_median_ms"] <= row["parent_median_ms"] + row["parent_spread_ms"]
        res["calls"][call] = row
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    sys.exit(0 if all(r["no_regression"] for r in res["calls"].values()) else 1)


if __name__ == "__main__":
    main()
