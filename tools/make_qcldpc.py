#!/usr/bin/env python3
"""Generate the project's quasi-cyclic LDPC code family (lifting size Z = 64, 128 or 256, 24 block columns, rates 1/2,
2/3, 3/4, 5/6) and write gf3_audio_modem_amd/data/qcldpc_z<Z>.json (one [mb, 24] shift table per rate, -1 = zero block;
plain text, one block row per line, so the tables diff and review like source).  The base shape -- block rows, degree
profiles, parity part -- is the same for every Z; only the shifts, drawn in [0, Z), differ.

Construction (NumPy only, fixed seed):
  - parity part: dual-diagonal (the 802.11n shape) -- first parity column shifts (x, 0, x) at rows 0, mb/2, mb-1 with
    x = 1, the other parity columns bidiagonal with shift 0, so p0 = sum of the block rows' message parts and the
    other parity blocks follow by recursion (linear-time encoding, no inversion);
  - message part: column degrees from a small per-rate profile (>= 3), rows picked to keep the row degrees even, and
    every shift drawn at random among the values that close no 4-cycle with the blocks already placed (a column that
    cannot be placed restarts the whole table from the next draw of the same generator).
Every property is then asserted by tests/ldpc_ref.check_properties (Z = 64; the same checks tests/test_ldpc_cpu.py
makes) or tests/ldpc_ref_z.check_properties (Z > 64; tests/test_ldpc_wide_cpu.py) and printed.  The output is
deterministic: rerunning this script reproduces the committed tables (--check compares them).

    python tools/make_qcldpc.py [--Z {64,128,256}] [--check]     (--check: verify the committed file instead of writing it)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ldpc_ref, ldpc_ref_z  # noqa: E402

NB = 24
SEEDS = {64: 20261016, 128: 20261017, 256: 20261017}      # one generator per lifting size


def out_path(Z):
    return os.path.join(ROOT, "gf3_audio_modem_amd", "data", f"qcldpc_z{Z}.json")


# rate -> (block rows, message-column degrees); higher-degree columns first (they protect the weak degree-2 parity)
PROFILE = {
    "1/2": (12, [8, 8, 6, 6] + [3] * 8),
    "2/3": (8, [6, 6, 4, 4] + [3] * 12),
    "3/4": (6, [4, 4, 4, 4] + [3] * 14),
    "5/6": (4, [3] * 20),
}


def parity_part(mb):
    sh = np.full((mb, mb), -1, dtype=np.int64)
    sh[0, 0] = sh[mb - 1, 0] = 1
    sh[mb // 2, 0] = 0
    for c in range(1, mb):
        sh[c - 1, c] = sh[c, c] = 0
    return sh


def closes_4cycle(sh, i, j, s, Z):
    """Would shift s at (i, j) close a 4-cycle with the non-zero blocks of sh?"""
    mb, nb = sh.shape
    for i2 in range(mb):
        if i2 == i or sh[i2, j] < 0:
            continue
        for j2 in range(nb):
            if j2 == j or sh[i, j2] < 0 or sh[i2, j2] < 0:
                continue
            if (s - sh[i, j2] + sh[i2, j2] - sh[i2, j]) % Z == 0:
                return True
    return False


def build(mb, degs, rng, Z, tries=200):
    kb = NB - mb
    assert len(degs) == kb
    for _ in range(tries):
        sh = np.full((mb, NB), -1, dtype=np.int64)
        sh[:, kb:] = parity_part(mb)
        row_deg = (sh >= 0).sum(axis=1).astype(float)
        ok = True
        for j in range(kb):
            # the degs[j] least loaded rows, random tie-break
            order = np.lexsort((rng.random(mb), row_deg))
            rows = np.sort(order[:degs[j]])
            for i in rows:
                cand = [s for s in rng.permutation(Z) if not closes_4cycle(sh, i, j, s, Z)]
                if not cand:
                    ok = False
                    break
                sh[i, j] = cand[0]
                row_deg[i] += 1
            if not ok:
                break
        if ok:
            return sh.astype(np.int16)
    raise RuntimeError(f"no 4-cycle-free table found for mb={mb}")


def generate(Z=64):
    rng = np.random.default_rng(SEEDS[Z])
    return {rate: build(mb, degs, rng, Z) for rate, (mb, degs) in PROFILE.items()}


def check_properties(sh, Z, **kw):
    return ldpc_ref.check_properties(sh, **kw) if Z == 64 else ldpc_ref_z.check_properties(sh, Z, **kw)


def dumps(tabs, Z=64):
    """{"Z": 64, "nb": 24, "rates": {rate: [[shift, ...] per block row]}}, one block row per line."""
    lines = ['{', f' "Z": {Z},', f' "nb": {NB},', ' "rates": {']
    w = len(str(Z - 1))
    for r, (rate, sh) in enumerate(tabs.items()):
        rows = [" [" + ", ".join(f"{int(v):{w}d}" for v in row) + "]" for row in sh]
        lines.append(f'  "{rate}": [\n  ' + ",\n  ".join(rows) + "\n  ]" + ("," if r < len(tabs) - 1 else ""))
    lines += [' }', '}']
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Z", type=int, choices=sorted(SEEDS), default=64)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    Z, out = a.Z, out_path(a.Z)
    tabs = generate(Z)
    for rate, sh in tabs.items():
        mb = sh.shape[0]
        print(f"rate {rate}: mb={mb} nb={NB} n={NB * Z} k={(NB - mb) * Z}, row degrees {(sh >= 0).sum(axis=1).tolist()}")
        for line in check_properties(sh, Z, seed=1):
            print("   ", line)
    if a.check:
        assert open(out).read() == dumps(tabs, Z), f"{out} differs from the generator's output"
        print("committed tables match the generator")
        return
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(dumps(tabs, Z))
    print("wrote", out)


if __name__ == "__main__":
    main()
