#!/usr/bin/env python3
"""Throughput of the QC-LDPC kernels (csrc/gf3rx_ldpc.hip) per rate, one JSON line.

    python tools/time_ldpc.py [--n-cw 65536] [--reps 5] [--max-iter 10] [--Z {128,256}]

decode_full: max_iter iterations on every codeword -- the input is pure noise, so no codeword satisfies its checks and
             early termination never fires (every iteration count is checked to be -max_iter);
decode_clean: noiseless +-8 LLRs of valid codewords -- every codeword stops after its first iteration;
encode:      message bits -> codewords.
Rates are coded bits (n per codeword) and information bits (k) per second, from the median of `reps` event-timed
launches after one warm-up launch.

--Z: time the codes of that lifting size (n = 24 Z) beside the Z = 64 ones in the same process, on the same number of
coded bits (n_cw is the number of Z = 64 codewords: 64 n_cw / Z codewords of the longer code), and also write the
result to profiles/ldpc_wide_time.json."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd import QCLDPC  # noqa: E402
from gf3_audio_modem_amd.ldpc import RATES  # noqa: E402


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


def time_family(a, dev, Z, n_cw):
    """{rate: {decode_full, decode_clean, encode}} of the family of lifting size Z on n_cw codewords per launch."""
    g = torch.Generator(device=dev).manual_seed(1)
    out = {}
    for rate in RATES:
        q = QCLDPC(rate, dev, Z=Z)
        msg = torch.randint(0, 2, (n_cw, q.k), dtype=torch.uint8, device=dev, generator=g)
        cw = q.encode(msg)
        clean = (1.0 - 2.0 * cw.float()) * 8.0
        noise = torch.randn((n_cw, q.n), device=dev, generator=g) * 4.0
        r = {}
        for name, llr in (("decode_full", noise), ("decode_clean", clean)):
            bits, its = q.decode(llr, max_iter=a.max_iter, want_iters=True)
            its = its.cpu().numpy()
            if name == "decode_full":
                assert (its == -a.max_iter).all(), "a noise codeword converged: early termination was not forced off"
            else:
                assert (its == 1).all() and torch.equal(bits, msg), "clean codewords must decode in one iteration"
            ms = ev_ms(lambda: q.decode(llr, max_iter=a.max_iter), a.reps)
            r[name] = {"ms": ms, "iterations": int(np.abs(its).mean()), "coded_Gbps": n_cw * q.n / ms / 1e6,
                       "info_Gbps": n_cw * q.k / ms / 1e6}
        ms = ev_ms(lambda: q.encode(msg), a.reps)
        r["encode"] = {"ms": ms, "coded_Gbps": n_cw * q.n / ms / 1e6, "info_Gbps": n_cw * q.k / ms / 1e6}
        out[rate] = r
        q.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-cw", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--Z", type=int, choices=(128, 256), default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"n_cw": a.n_cw, "max_iter": a.max_iter, "device": torch.cuda.get_device_name(dev),
           "rates": time_family(a, dev, 64, a.n_cw)}
    if a.Z:
        n_cw = a.n_cw * 64 // a.Z
        assert n_cw * a.Z == a.n_cw * 64, "--n-cw must be a multiple of Z / 64"
        res["wide"] = {"Z": a.Z, "n_cw": n_cw, "rates": time_family(a, dev, a.Z, n_cw)}
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "ldpc_wide_time.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
