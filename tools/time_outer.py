#!/usr/bin/env python3
"""Cost of the outer Reed-Solomon erasure code (csrc/gf3rx_outer.hip), one JSON line, also written to
profiles/outer_time.json (GF3_PROFILE_DIR=<dir>: there instead).

    python tools/time_outer.py [--codewords 65536] [--reps 7]

65 536 codewords of rate 1/2 at Z = 64 (k = 768 message bits, one byte per bit), (G, R) = (20, 4): 2730 groups.
Event-timed medians of `reps` after one warm-up, every timed window holding INNER back-to-back launches (one launch is
tens of microseconds).  Three legs: encode; recover with no erasure (a pass over the iteration counts only); recover with
one erased data member in every group.  Each is reported as the bytes the algorithm must move per second, next to a
device-to-device copy that moves the same number of bytes (half read, half written), timed in the same process."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd import OuterRS  # noqa: E402
from tools.time_noise import ev_ms  # noqa: E402

INNER = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codewords", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    G, R, k = 20, 4, 768
    NG = a.codewords // (G + R)
    rs = OuterRS(G, R, k)
    dev = rs.device
    g = torch.Generator(device=dev).manual_seed(1)
    msg = torch.randint(0, 2, (NG * G, k), device=dev, generator=g, dtype=torch.uint8)
    par = rs.encode(msg)
    sent = torch.cat([msg.reshape(NG, G, k).transpose(0, 1), par.reshape(NG, R, k).transpose(0, 1)]).contiguous().reshape(-1, k)
    good = torch.full(((G + R) * NG,), 3, dtype=torch.int32, device=dev)
    one = good.clone()
    member = torch.randint(0, G, (NG,), device=dev, generator=g)
    one[member * NG + torch.arange(NG, device=dev)] = -50
    bits = sent.clone()
    _, status = rs.recover(bits, one)
    assert torch.equal(bits, sent) and bool((status == 1).all())              # (repairing intact rows rewrites what they hold)
    flags = (G + R) * NG * 4 + NG * 4
    legs = {
        "encode": (lambda: rs.encode(msg), NG * (G + R) * k),
        "recover_no_erasure": (lambda: rs.recover(bits, good), flags),
        "recover_one_per_group": (lambda: rs.recover(bits, one), flags + NG * (G + 1) * k),
    }
    res = {"codewords": NG * (G + R), "groups": NG, "G": G, "R": R, "k": k, "reps": a.reps, "launches_per_window": INNER,
           "device": torch.cuda.get_device_name(dev)}
    for name, (fn, by) in legs.items():
        def window(fn=fn):
            for _ in range(INNER):
                fn()
        src = torch.empty(max(by // 2, 1), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        def copies(src=src, dst=dst):
            for _ in range(INNER):
                dst.copy_(src)
        ms, ms_copy = ev_ms(window, a.reps) / INNER, ev_ms(copies, a.reps) / INNER
        res[name] = {"ms": ms, "bytes": by, "GBps": by / ms / 1e6, "copy_ms": ms_copy, "copy_GBps": by / ms_copy / 1e6}
    line = json.dumps(res)
    print(line)
    out = os.environ.get("GF3_PROFILE_DIR") or os.path.join(ROOT, "profiles")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "outer_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
