#!/usr/bin/env python3
"""Same-box timing of the launch-bound stream sync (the small kernels weigh most here): sync_stream on a ~3 M-sample f32 stream (reference geometry, 3 packets + terminating chirp), modes 1 and 2.
Wall time per call (the call ends with its own stream synchronise): median of 300 (or argv[1]) calls after 30 warm-ups.  GF3_LIB selects the build."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from gf3_audio_modem_amd import Engine, RxConfig
known = np.unpackbits(np.load(os.path.join(ROOT, "gf3_audio_modem_amd", "data", "known_bits.npz"))["packed"])
cfg = RxConfig(data_bins=np.arange(100, 1500), known_bits=np.tile(known, 2), in_dtype=torch.float32)
eng = Engine(cfg)
gen = torch.Generator(device="cuda").manual_seed(1)
F = 3
packed = torch.randint(0, 256, (F, eng.bytes_per_frame), dtype=torch.uint8, device="cuda", generator=gen)
rows = eng.tx_frames(packed, np.zeros(cfg.K, dtype=complex), out_dtype=torch.float32)
x = torch.cat([rows.reshape(-1), torch.from_numpy(eng.chirp_replica()).float().cuda(), torch.zeros(60000, device="cuda")])
x = x + 0.01 * torch.randn(x.shape, device="cuda", generator=gen)
res = {"n": int(x.numel())}
for mode in (1, 2):
    for _ in range(30):
        p = eng.sync_stream(x, mode=mode)
    torch.cuda.synchronize()
    ts = []
    for _ in range(int(sys.argv[1]) if len(sys.argv) > 1 else 300):
        t0 = time.perf_counter(); p = eng.sync_stream(x, mode=mode); ts.append(time.perf_counter() - t0)
    res[f"mode{mode}_ms"] = float(np.median(ts) * 1e3)
    res[f"mode{mode}_peaks"] = int(p.numel())
print(json.dumps(res))
