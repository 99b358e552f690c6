#!/usr/bin/env python3
"""Cost of the per-codeword CRC-32 (csrc/gf3rx_crc.hip), one JSON line, also written to profiles/crc_time.json
(GF3_PROFILE_DIR=<dir>: there instead).

    python tools/time_crc.py [--codewords 65536] [--reps 7]

65 536 codewords at k = 768 (rate 1/2, Z = 64) and k = 5120 (rate 5/6, Z = 256), one byte per bit.  Event-timed medians of
`reps` after one warm-up, every timed window holding INNER back-to-back launches into preallocated outputs (one launch is
tens of microseconds: a window of one would time the host's enqueue).  Per k: attach (k - 32 bytes read, k written per
codeword) and check with every output (k read, k - 32 + 1 + 4 written, 4 read), each next to a device-to-device copy of
the same number of bytes (half read, half written), and next to gf3_ldpc_decode of the same codewords on noiseless LLRs
-- one iteration each, the cheapest decode there is -- timed in the same process."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd import QCLDPC, CodewordCRC, _lib  # noqa: E402
from tools.time_noise import ev_ms  # noqa: E402

CODES = ((768, "1/2", 64), (5120, "5/6", 256))
INNER = 10


def window(fn):
    def run():
        for _ in range(INNER):
            fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codewords", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    n_cw = a.codewords
    res = {"codewords": n_cw, "reps": a.reps, "launches_per_window": INNER, "device": torch.cuda.get_device_name(torch.cuda.current_device())}
    for k, rate, Z in CODES:
        code = QCLDPC(rate, Z=Z)
        assert code.k == k
        crc = CodewordCRC(k)
        dev = crc.device
        g = torch.Generator(device=dev).manual_seed(k)
        payload = torch.randint(0, 2, (n_cw, k - 32), device=dev, generator=g, dtype=torch.uint8)
        msg = crc.attach(payload)
        llr = 4.0 * (1.0 - 2.0 * code.encode(msg).float())
        dec, iters = code.decode(llr, max_iter=10, want_iters=True)
        back, bad, _ = crc.check(dec, iters)
        assert torch.equal(dec, msg) and bool((iters == 1).all()) and not bool(bad.any()) and torch.equal(back, payload)
        by_attach = n_cw * (2 * k - 32)
        by_check = n_cw * (2 * k - 32 + 1 + 8)
        row = {"rate": rate, "Z": Z, "n": code.n}
        lib, st, ptr = crc.lib, _lib.stream(dev), _lib.ptr
        out_msg, out_pay, out_bad = torch.empty_like(msg), torch.empty_like(payload), torch.empty_like(bad)
        legs = (("attach", lambda: lib.gf3_crc_attach(ptr(payload), n_cw, k, ptr(out_msg), st), by_attach),
                ("check", lambda: lib.gf3_crc_check(ptr(msg), n_cw, k, ptr(out_pay), ptr(iters), ptr(out_bad), st), by_check))
        for name, fn, by in legs:
            assert fn() == 0
            src = torch.empty(by // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            ms, ms_copy = ev_ms(window(fn), a.reps) / INNER, ev_ms(window(lambda: dst.copy_(src)), a.reps) / INNER
            row[name] = {"ms": ms, "bytes": by, "GBps": by / ms / 1e6, "copy_ms": ms_copy, "copy_GBps": by / ms_copy / 1e6,
                         "over_copy": ms / ms_copy}
        assert torch.equal(out_msg, msg) and torch.equal(out_pay, payload) and not bool(out_bad.any())
        ms_dec = ev_ms(window(lambda: code.decode(llr, max_iter=10, want_iters=True)), a.reps) / INNER
        row["decode_1_iteration_ms"] = ms_dec
        row["check_over_decode"] = row["check"]["ms"] / ms_dec
        row["attach_over_decode"] = row["attach"]["ms"] / ms_dec
        res[f"k{k}"] = row
    line = json.dumps(res)
    print(line)
    out = os.environ.get("GF3_PROFILE_DIR") or os.path.join(ROOT, "profiles")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "crc_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
