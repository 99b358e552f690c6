#!/usr/bin/env python3
"""SHA-256 of everything the demodulator hands back, on seeded inputs: two builds that print the same JSON compute the same
bits (GF3_LIB selects the build).  N = 1024 and 4096; f32, i16 and f64 storage; QPSK and 16-QAM; D = 5 and 8, P = 2, F = 5 with
one ragged packet; clean and with noise at 10 dB (some packets go to the fp64 pass); demod_frames one-launch and two-phase,
screened and all-fp64, bits only and every dump; demod_frames_llr with both weights; equalise."""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from gf3_audio_modem_amd import Engine, RxConfig, qpsk_table, square_qam_table
known = np.unpackbits(np.load(os.path.join(ROOT, "gf3_audio_modem_amd", "data", "known_bits.npz"))["packed"])

def sha(o):
    return {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16] for k, v in sorted(o.items()) if torch.is_tensor(v)}

FULL = ("eq", "Hs", "He", "slope", "Hest", "status")
out, F, P = {}, 5, 2
for N in (1024, 4096):
    K = N // 2 - 1
    for cname, (pts, bt) in (("qpsk", qpsk_table()), ("qam16", square_qam_table(4))):
        for D in (5, 8):
            for dname, dt in (("f32", torch.float32), ("i16", torch.int16), ("f64", torch.float64)):
                cfg = RxConfig(N=N, CP=N // 8, P=P, D=D, data_bins=np.arange(1, K + 1), const_points=pts, const_bits=bt, known_bits=np.tile(known, 2), in_dtype=dt)
                eng = Engine(cfg)
                gen = torch.Generator(device="cuda").manual_seed(N + D)
                packed = torch.randint(0, 256, (F, eng.bytes_per_frame), dtype=torch.uint8, device="cuda", generator=gen)
                rows = eng.tx_frames(packed, np.zeros(K, dtype=complex), out_dtype=torch.float64).reshape(-1)
                starts = torch.arange(F, device="cuda") * cfg.frame_len + cfg.chirp_length
                starts[F - 1] += cfg.frame_len                               # the last packet runs off the end: ragged
                for nname, sigma in (("clean", 0.0), ("snr10", 10 ** -0.5)):
                    x = rows + torch.randn(rows.shape, device="cuda", dtype=torch.float64, generator=gen) * (sigma * float(rows[int(starts[0]):].pow(2).mean().sqrt()))
                    x = (x * (8000.0 / float(x.abs().max()))).round().to(dt) if dt == torch.int16 else x.to(dt)
                    key = f"N{N}/{cname}/D{D}/{dname}/{nname}"
                    for split in (False, True):
                        for prec in (None, "fp64"):
                            for want in ((), FULL):
                                out[f"{key}/frames split={split} precision={prec} want={len(want)}"] = sha(eng.demod_frames(x, starts, want=want, split=split, precision=prec))
                        for w in ("csi", "none"):
                            out[f"{key}/llr split={split} weight={w}"] = sha(eng.demod_frames_llr(x, starts, weight=w, split=split, want=("Hs", "He", "slope", "status")))
                    if dt == torch.float64:
                        sp = torch.randn((F, 2 * P + D, K, 2), device="cuda", dtype=torch.float64, generator=gen)
                        sp = torch.view_as_complex(sp)
                        out[f"{key}/equalise"] = sha(eng.equalise(sp[:, 2 * P:], sp[:, :P], sp[:, P:2 * P], want=("Hest",)))
                eng.close()
print(json.dumps(out, sort_keys=True))
