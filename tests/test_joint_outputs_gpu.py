"""Every call of the two-speaker paths against what the commit before the consolidation of their host side (gf3rx_joint.h,
with_branches and tile_grid of gf3rx_host.h) gave on the MI355X: SHA-256 digests of each output tensor's bytes next to the
digest of the inputs it was computed from (tests/golden/joint_outputs.json: case -> item -> [inputs, output]), built like
tests/test_soft_outputs_gpu.py.  A changed generator shows as a changed input digest, a changed kernel or a changed launch
(branch dispatch, grid, argument block) as a changed output digest.  That commit left every kernel's machine code as it
was, so what the digests held it to is the host side; they stand for the day the kernels' bodies are shared.  A float32
LLR hides most last-bit differences of the fp64 arithmetic behind it: one instantiation built from shared pieces differed
in 3 of 1.4 million LLRs, at the large F only.  Every kernel here documents a fixed summation order; the parent was
recorded twice, in two processes, and every item came out the same in both: all of them are held exactly.

    PYTHONPATH=TREE python tests/test_joint_outputs_gpu.py --record OUT.json      (TREE: a built checkout to record)
    python tests/test_joint_outputs_gpu.py --merge A.json B.json tests/golden/joint_outputs.json

Contexts: tests.tables.params_for(table, 1024, carriers, P=4, D=10, CP=64) with the fit range [10, 300) -- P = 4 so that
mimo_pilot_noise is legal, D = 10 even for the pairs, five pairs an odd last run -- for C = 70 (descending bins: one
partial 256-carrier tile) and C = 300 (ascending: two tiles, the second partial), on qpsk_ref and qpsk_rot (a 4-point
table that is no grid).
Packets: F = 3 and, for the detectors with B = 2, the smallest F at which the symbols-per-workgroup rule
(nchunk = ceil(8 n_cu / per) clamped to [1, units], run = ceil(units / nchunk)) gives a run >= 2 that does not divide the
streamed units for BOTH the D symbols of mimo_detect and the D / 2 pairs of stbc_detect: computed from the engine's n_cu,
asserted in the test (256 compute units: F = 512 on one tile and 256 on two, runs 3, 3, 3, 1 and pairs 2, 2, 1).
Inputs are built on the host from np.random.RandomState and uploaded.  Planted, one kind per packet so that the
neighbours show they are untouched:
  packet 0: in branch 0 a NaN and an infinite spectrum value; a NaN spectrum value in every branch at one cell;
  packet 1: a NaN estimate in branch 0, an infinite one in branch 1; weights 0, +Inf and NaN in branch 0 and 0 in every
            branch at one carrier; for joint_noise_weights a NaN variance (branch 0) and an infinite one;
  packet 2: a slope that is not finite (mimo_detect: branch 0's; stbc_detect: the one slope); for joint_noise_weights
            variances all 0 (a flat packet).
The pilot calls run on float64 and float32 samples with one offset off either end of the samples.  The known-bit detector
runs on an all-zero `known` plane, a random half-known one, and the same planes at an odd byte address."""
import dataclasses
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "joint_outputs.json")
N, CP, P, D = 1024, 64, 4, 10
K, NB = N // 2 - 1, N // 2 + 1
LEFT_OUT = []                                   # "case/item" that the parent's two recordings disagreed on: not in the golden file
CASES = [f"{t}-C{C}" for t in ("qpsk_ref", "qpsk_rot") for C in (70, 300)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bins_of(C):
    return np.arange(20 + C - 1, 19, -1) if C == 70 else np.arange(20, 20 + C)


def units_per_group(n_cu, per, units):
    """The library's rule: about 8 workgroups per compute unit, `per` of them per chunk of streamed units."""
    nchunk = min(max(-(-8 * n_cu // per), 1), units)
    return -(-units // nchunk)


def large_F(n_cu, ntile):
    """Smallest F > 3 at which the symbol run and the pair run are both at least 2 and leave a shorter last run."""
    for F in range(4, 8 * n_cu + 1):
        Dc, Jc = units_per_group(n_cu, F * ntile, D), units_per_group(n_cu, F * ntile, D // 2)
        if Dc >= 2 and D % Dc and Jc >= 2 and (D // 2) % Jc:
            return F, Dc, Jc
    raise AssertionError("no such F")


def cn(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


def detector_inputs(case, C, F, B):
    """Host arrays of one (case, F): B branches' spectra [F*D, N/2+1], estimates [F, 2, 2, K], slopes [F], weights [B, F, C]"""
    rs = np.random.RandomState(zlib.crc32(f"{case}-detect-{F}".encode()))
    bins = bins_of(C)
    x = {}
    for b in range(B):
        x[f"Y{b}"] = cn(rs, F * D, NB)
        H = cn(rs, F, 2, 2, K) * 0.7
        H[:, 1] = H[:, 0] * (1 + 0.3 * rs.randn(F, 2, K)) * np.exp(0.2j * rs.randn(F, 2, K))
        x[f"H{b}"] = H
        x[f"slope{b}"] = 3e-3 * rs.randn(F)
    w = np.exp(1.5 * rs.randn(B, F, C))
    w[rs.rand(B, F, C) < 0.02] = 0.0
    cell = lambda f, l: f * D + l
    x["Y0"][cell(0, 3), bins[17]] = complex(np.nan, 0.0)
    x["Y0"][cell(0, 4), bins[33]] = complex(1.0, np.inf)
    for b in range(B):
        x[f"Y{b}"][cell(0, 7), bins[50]] = complex(np.nan, np.nan)
    x["H0"][1, 1, 1, bins[40] - 1] = complex(0.0, np.nan)
    if B > 1:
        x["H1"][1, 0, 0, bins[41] - 1] = complex(np.inf, 0.0)
    w[0, 1, 60], w[0, 1, 61], w[0, 1, 62], w[:, 1, 63] = 0.0, np.inf, np.nan, 0.0
    x["slope0"][2] = np.inf
    stbc_slope = 3e-3 * rs.randn(F)
    stbc_slope[2] = np.nan
    x["slope"], x["w"] = stbc_slope, w
    return x


def known_planes(case, C, F):
    """`bits` and `known` [F, 2, D, C, 2] bytes: half the bits known, the known ones at random (non-zero bytes of any value)"""
    rs = np.random.RandomState(zlib.crc32(f"{case}-known".encode()))
    n = F * 2 * D * C * 2
    bits = (rs.randint(0, 2, n) * rs.randint(1, 256, n)).astype(np.uint8)
    known = ((rs.rand(n) < 0.5) * rs.randint(1, 256, n)).astype(np.uint8)
    return bits, known


def pilot_inputs(case):
    """Samples and offsets: three packet bodies inside the samples, one offset off either end"""
    rs = np.random.RandomState(zlib.crc32(f"{case}-pilots".encode()))
    body = (2 * P + D) * (N + CP)
    n = 100 + 3 * body + 300
    off = np.array([-1, 100, 100 + body + 7, n - body + 1, n - body], dtype=np.int64)
    return rs.randn(n), off


def variance_inputs(case, C):
    rs = np.random.RandomState(zlib.crc32(f"{case}-var".encode()))
    col = bins_of(C) - 1
    x = {f"var{b}": rs.chisquare(4, size=(3, 2, K)) * 10.0 ** rs.uniform(-3, 1, size=(1, 1, K)) for b in range(4)}
    x["var0"][1, 1, col[17]] = np.nan
    x["var0"][1, 0, col[C - 3]] = np.inf
    for b in range(4):
        x[f"var{b}"][2] = 0.0
    return x


class Recorder:
    """item -> [digest of the named inputs' digests, digest of the output]."""

    def __init__(self):
        self.din, self.items = {}, {}

    def take(self, arrays):
        self.din.update({k: sha(v) for k, v in arrays.items()})

    def put(self, item, used, out):
        key = hashlib.sha256(" ".join(self.din[k] for k in used).encode()).hexdigest()
        self.items[item] = [key, sha(out.cpu().numpy())]


def run(case):
    import torch
    from tests import tables as T
    from tests.util import engine_for
    table, C = case.rsplit("-C", 1)
    C = int(C)
    p = dataclasses.replace(T.params_for(table, N, bins_of(C), P=P, D=D, CP=CP), fit_lo=10, fit_hi=300)
    eng = engine_for(p)
    rec = Recorder()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    # ---- the pilot calls: float64 and float32 samples
    samples, off = pilot_inputs(case)
    for name, dtype in (("f64", np.float64), ("f32", np.float32)):
        e = eng if name == "f64" else engine_for(p, in_dtype=torch.float32)
        x = samples.astype(dtype)
        rec.take({f"x-{name}": x, "off": off})
        xd = dev(x)
        H, status = e.mimo_pilots(xd, off)
        assert status.cpu().numpy().tolist() == [1, 0, 0, 1, 0]
        var, vstatus = e.mimo_pilot_noise(xd, off, H)
        for item, out in (("mimo_pilots/H", H), ("mimo_pilots/status", status), ("mimo_pilot_noise/var", var),
                          ("mimo_pilot_noise/status", vstatus)):
            rec.put(f"{name}/{item}", (f"x-{name}", "off"), out)
        if e is not eng:
            e.close()

    # ---- the weights
    v = variance_inputs(case, C)
    rec.take(v)
    for B in (1, 2, 3, 4):
        used = [f"var{b}" for b in range(B)]
        rec.put(f"F3/joint_noise_weights/B{B}", used, eng.joint_noise_weights([dev(v[k]) for k in used]))

    # ---- the slope and the detectors, F = 3
    F = 3
    x = detector_inputs(case, C, F, 4)
    bits, known = known_planes(case, C, F)
    zero = np.zeros_like(known)
    x.update(bits=bits, known=known, zero=zero)
    rec.take(x)
    d = {k: dev(a) for k, a in x.items()}
    shifted = {}
    for k in ("bits", "known"):                             # the same planes at an odd byte address
        buf = torch.empty(x[k].size + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = d[k]
        shifted[k] = buf[1:]
        assert shifted[k].data_ptr() % 2 == 1 and shifted[k].is_contiguous()
    for B in (1, 2, 3, 4):
        Ys, Hs, sl = ([d[f"{k}{b}"] for b in range(B)] for k in ("Y", "H", "slope"))
        nY, nH, nS = ([f"{k}{b}" for b in range(B)] for k in ("Y", "H", "slope"))
        wB = d["w"][:B].contiguous()
        if B != 3:
            rec.put(f"F3/stbc_slope/B{B}", nH, eng.stbc_slope(Hs))
        for tag, kw, more in (("plain", {}, []), ("weighted", dict(weights=wB), ["w"])):
            rec.put(f"F3/mimo_detect/B{B}/{tag}", nY + nH + nS + more, eng.mimo_detect(Ys, Hs, sl, **kw))
            rec.put(f"F3/stbc_detect/B{B}/{tag}", nY + nH + ["slope"] + more, eng.stbc_detect(Ys, Hs, d["slope"], **kw))
            if B != 3:
                for plane, bt, kn, names in (("zero", d["bits"], d["zero"], ["bits", "zero"]),
                                             ("half", d["bits"], d["known"], ["bits", "known"]),
                                             ("odd", shifted["bits"], shifted["known"], ["bits", "known"])):
                    rec.put(f"F3/mimo_detect_known/B{B}/{tag}/{plane}", nY + nH + nS + more + names,
                            eng.mimo_detect_known(Ys, Hs, sl, bt, kn, **kw))
    del d, shifted

    # ---- the detectors at the F whose runs leave a shorter last one, B = 2
    ntile = -(-C // 256)
    F, Dc, Jc = large_F(eng.n_cu, ntile)
    assert Dc >= 2 and D % Dc and Jc >= 2 and (D // 2) % Jc
    assert units_per_group(eng.n_cu, F * ntile, D) == Dc and units_per_group(eng.n_cu, F * ntile, D // 2) == Jc
    x = detector_inputs(case, C, F, 2)
    big = Recorder()
    big.take(x)
    d = {k: dev(a) for k, a in x.items()}
    Ys, Hs, sl = ([d[f"{k}{b}"] for b in range(2)] for k in ("Y", "H", "slope"))
    for tag, kw, more in (("plain", {}, []), ("weighted", dict(weights=d["w"]), ["w"])):
        big.put(f"Fbig/mimo_detect/B2/{tag}", ["Y0", "Y1", "H0", "H1", "slope0", "slope1"] + more, eng.mimo_detect(Ys, Hs, sl, **kw))
        big.put(f"Fbig/stbc_detect/B2/{tag}", ["Y0", "Y1", "H0", "H1", "slope"] + more, eng.stbc_detect(Ys, Hs, d["slope"], **kw))
    del d
    eng.close()
    return {**rec.items, **big.items}


@pytest.mark.parametrize("case", CASES)
def test_case_gives_what_the_parent_gave(case):
    want = json.load(open(GOLD))[case]
    got = run(case)
    assert set(want) <= set(got)
    assert sorted(f"{case}/{k}" for k in set(got) - set(want)) == sorted(k for k in LEFT_OUT if k.startswith(case + "/"))
    assert [k for k in want if got[k][0] != want[k][0]] == [], "the inputs changed: the generator, not a kernel"
    assert [k for k in want if got[k][1] != want[k][1]] == []


def main(argv):
    if argv[0] == "--record":
        out = {}
        for case in CASES:
            out[case] = run(case)
            print(f"{case}: {len(out[case])} items", flush=True)
        json.dump(out, open(argv[1], "w"), indent=0, sort_keys=True)
    elif argv[0] == "--merge":
        a, b = json.load(open(argv[1])), json.load(open(argv[2]))
        assert sorted(a) == sorted(b) and all(sorted(a[c]) == sorted(b[c]) for c in a)
        differ = [(c, k) for c in a for k in a[c] if a[c][k] != b[c][k]]
        print("items that differ between the two recordings:", differ)
        print("not reproducible on the recorded tree itself: a finding about that tree; left out, to be named in LEFT_OUT" if differ else "all held")
        with open(argv[3], "w") as fh:
            json.dump({c: {k: v for k, v in a[c].items() if (c, k) not in differ} for c in a}, fh, indent=0, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
