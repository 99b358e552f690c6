#!/usr/bin/env python3
"""Cost of the decoder feedback (csrc/gf3rx_feedback.hip), one JSON line, written to profiles/feedback_time.json.

    python tools/time_feedback.py [--packets 256 3] [--reps 7] [--out profiles/feedback_time.json]

Geometry and repetition scheme of tools/time_track.py: mode A2 (D = 180, C = 1400, QPSK), "QCLDPC-1/2" codewords laid
out over the packets, noisy equalised symbols, event-timed medians after one warm-up launch.  Timed in one process, on
the same eq, for each packet count: feedback_equalise at the default window (2, 8) and at the largest one (8, 64), with
nine codewords in ten trusted; a device copy of the same eq bytes (the yardstick of the other time_*.py tools); the
first pass of the noise-weighted chain (noise estimate, demapper, decode of every codeword) and one whole extra pass
(re-encode, the two planes, feedback_equalise, noise estimate, demapper, decode of the untrusted tenth).  Nothing here
has a parent to be faster than: no ratio is promised, the numbers are reported."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd.OFDM import _qcldpc_code, receiver  # noqa: E402
from tools.time_noise import ev_ms  # noqa: E402


def one(eng, code, F, reps, max_iter=50):
    cfg = eng.cfg
    D, C, mu = cfg.D, cfg.C, cfg.mu
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(1)
    per = D * C * mu
    n_cw = F * per // code.n
    full = torch.randint(0, 2, (n_cw, code.k), device=dev, generator=g, dtype=torch.uint8)
    coded = torch.randint(0, 2, (F * per,), device=dev, generator=g, dtype=torch.uint8)
    coded[: n_cw * code.n] = code.encode(full).reshape(-1)
    b = coded.reshape(-1, 2).double()                               # the reference's QPSK: (b0, b1) -> ((1 - 2 b1) + i (1 - 2 b0)) / sqrt 2
    n = F * D * C
    noise = lambda: 0.3 * torch.randn(n, device=dev, generator=g, dtype=torch.float64)
    eq = torch.complex((1 - 2 * b[:, 1]) / np.sqrt(2) + noise(), (1 - 2 * b[:, 0]) / np.sqrt(2) + noise()).reshape(F * D, C)
    trusted = (torch.rand(n_cw, device=dev, generator=g) >= 0.1).to(torch.uint8)
    untrusted = torch.nonzero(trusted == 0).reshape(-1)

    def planes():
        out = []
        for rows in (code.encode(full * trusted[:, None]), trusted[:, None].expand(n_cw, code.n)):
            plane = torch.zeros(F * per, dtype=torch.uint8, device=dev)
            plane[: n_cw * code.n] = rows.reshape(-1)
            out.append(plane)
        return out
    bits, known = planes()
    out = torch.empty_like(eq)
    llr = torch.empty(n * mu, dtype=torch.float32, device=dev)

    def weigh(e):
        return eng.soft_demap_nw(e, eng.noise_estimate(e), out=llr)

    def first_pass():
        return code.decode(weigh(eq)[: n_cw * code.n], max_iter=max_iter, want_iters=True)

    def extra_pass():
        bt, kn = planes()
        fb = eng.feedback_equalise(eq, bt, kn, out=out)
        return code.decode(weigh(fb)[: n_cw * code.n].reshape(n_cw, code.n)[untrusted], max_iter=max_iter, want_iters=True)
    _, gain = eng.feedback_equalise(eq, bits, known, want_gain=True)
    b_eq = n * 16
    by = 2 * b_eq + 2 * n * mu
    legs = {
        "feedback_equalise": (lambda: eng.feedback_equalise(eq, bits, known, out=out), by),
        "feedback_equalise_window_8_64": (lambda: eng.feedback_equalise(eq, bits, known, 8, 64, 4, out=out), by),
        "device_copy": (lambda: out.copy_(eq), 2 * b_eq),
        "first_pass": (first_pass, None),
        "extra_pass": (extra_pass, None),
    }
    res = {"packets": F, "codewords": n_cw, "untrusted": int(untrusted.numel()),
           "gains_used": int((gain != 1).sum()), "symbols": n}
    for name, (fn, nbytes) in legs.items():
        ms = ev_ms(fn, reps)
        res[name] = {"ms": ms} if nbytes is None else {"ms": ms, "bytes": nbytes, "GBps": nbytes / ms / 1e6}
    res["over_copy"] = res["feedback_equalise"]["ms"] / res["device_copy"]["ms"]
    res["window_8_64_over_copy"] = res["feedback_equalise_window_8_64"]["ms"] / res["device_copy"]["ms"]
    res["extra_over_first_pass"] = res["extra_pass"]["ms"] / res["first_pass"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, nargs="+", default=[256, 3])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feedback_time.json"))
    a = ap.parse_args()
    eng = receiver("A2", encoding="QCLDPC-1/2")._engine()
    code = _qcldpc_code("1/2", eng.device)
    cfg = eng.cfg
    res = {"D": cfg.D, "C": cfg.C, "mu": cfg.mu, "window": [2, 8], "min_known": 4, "reps": a.reps,
           "device": torch.cuda.get_device_name(eng.device), "compute_units": eng.n_cu,
           "runs": [one(eng, code, F, a.reps) for F in a.packets]}
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
