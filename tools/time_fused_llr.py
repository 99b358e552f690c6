#!/usr/bin/env python3
"""The coded receive path from samples to CSI-weighted LLRs, staged against fused, one JSON line.

    python tools/time_fused_llr.py [--reps 7] [--out profiles/fused_llr_time.json]

staged: demod_frames(want eq, Hs, He) + soft_demap_csi (MODE_FULL dump, soft demapper, csi_weight_kernel: three launches)
fused:  demod_frames_llr(weight="csi")                  (MODE_SOFT of the fused kernel: one launch)
on (a) 256 mode-A2 packets (D = 180, C = 1400; the geometry of tools/time_noise.py), reference QPSK and 16-QAM, and
(b) 4096 packets of the bench's config-2 geometry (N = 4096, CP = 512, P = 2, D = 8, C = 2046, QPSK); f32 samples
synthesised by gf3_tx_frames.  Event-timed medians of `reps` runs after one warm-up, in one process; the bytes each path
moves beyond the samples both read (eq 16 B written and read, LLRs 4 mu B written, read and rewritten, Hs / He read,
against 4 mu B written once) and the largest LLR difference of the two paths relative to the packet's largest LLR."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gf3_audio_modem_amd import Engine, RxConfig  # noqa: E402
from gf3_audio_modem_amd.engine import qpsk_table, square_qam_table  # noqa: E402


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


def leg(name, F, N, CP, P, D, bins, table, reps):
    pts, bt = table
    K, mu = N // 2 - 1, bt.shape[1]
    known = np.unpackbits(np.load(os.path.join(ROOT, "gf3_audio_modem_amd", "data", "known_bits.npz"))["packed"])
    known = np.tile(known, -(-K * mu // len(known)))
    cfg = RxConfig(N=N, CP=CP, P=P, D=D, data_bins=bins, const_points=pts, const_bits=bt, known_bits=known, in_dtype=torch.float32)
    eng = Engine(cfg)
    gen = torch.Generator(device="cuda").manual_seed(7)
    payload = torch.randint(0, 256, (F, eng.bytes_per_frame), dtype=torch.uint8, device="cuda", generator=gen)
    filler = np.full(K, pts[0], dtype=complex)
    x = eng.tx_frames(payload, filler, out_dtype=torch.float32)
    x += 0.05 * x.std() * torch.randn(x.shape, device="cuda", generator=gen, dtype=torch.float32)
    starts = torch.arange(F, device="cuda", dtype=torch.int64) * cfg.frame_len + cfg.chirp_length
    C = len(bins)
    n = F * D * C
    llr_s = torch.empty(n * mu, dtype=torch.float32, device="cuda")
    llr_f = torch.empty(n * mu, dtype=torch.float32, device="cuda")

    def staged():
        o = eng.demod_frames(x, starts, want=("eq", "Hs", "He"))
        eng.soft_demap_csi(o["eq"], o["Hs"], o["He"], out=llr_s)

    def fused():
        eng.demod_frames_llr(x, starts, weight="csi", out=llr_f)

    ms_s, ms_f = ev_ms(staged, reps), ev_ms(fused, reps)
    a, b = llr_s.view(F, -1).double(), llr_f.view(F, -1).double()
    rel = float(((a - b).abs().amax(dim=1) / a.abs().amax(dim=1)).max())
    by_s = n * 32 + 3 * n * mu * 4 + 3 * F * K * 16           # eq out + in, LLRs out / in / out, Hs / He out and in again
    by_f = n * mu * 4
    res = {"packets": F, "N": N, "D": D, "C": C, "mu": mu, "staged_ms": ms_s, "fused_ms": ms_f, "fused_over_staged": ms_f / ms_s,
           "staged_bytes": by_s, "fused_bytes": by_f, "max_llr_delta_over_packet_max": rel, "plan": eng.demod_plan(F)}
    eng.close()
    del x, llr_s, llr_f
    torch.cuda.empty_cache()
    return name, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--packets-a", type=int, default=256)
    ap.add_argument("--packets-b", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_llr_time.json"))
    a = ap.parse_args()
    a2 = dict(N=4096, CP=224, P=20, D=180, bins=np.arange(100, 1500))
    c2 = dict(N=4096, CP=512, P=2, D=8, bins=np.arange(1, 2047))
    res = {"reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for name, F, geo, table in (("a_modeA2_qpsk", a.packets_a, a2, qpsk_table()), ("a_modeA2_qam16", a.packets_a, a2, square_qam_table(4)),
                                ("b_config2_qpsk", a.packets_b, c2, qpsk_table())):
        k, v = leg(name, F, reps=a.reps, table=table, **geo)
        res[k] = v
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
