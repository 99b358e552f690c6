"""Event-timed: the QPSK demodulation of the headline batch, all-fp64 (precision="fp64") against the screened path (auto),
median of 20 after 3, with the number of packets the screen listed there (must be 0), and the listed share of the same
batch with white noise at 10 dB.  GF3_LIB selects the build."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import argparse, numpy as np, torch
import importlib.util
spec = importlib.util.spec_from_file_location("gf3_bench", os.path.join(ROOT, "bench.py")); bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
ap = argparse.ArgumentParser(); ap.add_argument("--frames", type=int, default=65536); ap.add_argument("--stride", type=int, default=78720); ap.add_argument("--window", type=int, default=320)
args = ap.parse_args()
eng, cfg, big, payload, gaps = bench.build_workload(args, 0)
F = args.frames
starts = torch.arange(F, device="cuda", dtype=torch.int64) * args.stride + gaps + cfg.chirp_length
bits = torch.empty((F, eng.bytes_per_frame), dtype=torch.uint8, device="cuda")
ms64 = bench._event_ms(lambda: eng.demod_frames(big, starts, out_bits=bits, split=False, precision="fp64"))
ok64 = bool(torch.equal(bits, payload)); bits.zero_()
ms32 = bench._event_ms(lambda: eng.demod_frames(big, starts, out_bits=bits, split=False))
path = eng.demod_frames_last()["path"]
ok32 = bool(torch.equal(bits, payload))
listed = int(eng.debug_demod_screen(big, starts)["listed"].numel())
out = {"fp64_ms": ms64, "screened_ms": ms32, "path": path, "fp64_exact": ok64, "screened_exact": ok32, "listed": listed}
# the same batch at 10 dB: what share of the packets goes to the fp64 pass, and what the call then costs
n_sym = (2 * cfg.P + cfg.D) * (cfg.N + cfg.CP)                   # (the level of the OFDM symbols: the chirp in front of them is louder)
rms = float(big.reshape(-1)[int(starts[0]): int(starts[0]) + n_sym].double().pow(2).mean().sqrt())
noisy = big + torch.randn(big.shape, device="cuda", dtype=torch.float32, generator=torch.Generator(device="cuda").manual_seed(3)) * (rms * 10 ** -0.5)
ref = eng.demod_frames(noisy, starts, split=False, precision="fp64")["bits"]
ms64n = bench._event_ms(lambda: eng.demod_frames(noisy, starts, out_bits=bits, split=False, precision="fp64"))
ms32n = bench._event_ms(lambda: eng.demod_frames(noisy, starts, out_bits=bits, split=False))
out["snr10"] = {"fp64_ms": ms64n, "screened_ms": ms32n, "equal": bool(torch.equal(bits, ref)),
                "listed_share": int(eng.debug_demod_screen(noisy, starts)["listed"].numel()) / F}
print(json.dumps(out))
