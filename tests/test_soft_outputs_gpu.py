"""Every soft-output call of the library against what the commit before the shared soft-output pieces gave on the MI355X:
SHA-256 digests of each output tensor's bytes next to the digest of the inputs it was computed from
(tests/golden/soft_outputs.json: case -> item -> [inputs, output]).  A changed generator shows as a changed input digest,
a changed kernel as a changed output digest.  Every kernel here documents a fixed summation order; the parent was recorded
twice, in two processes, and every item came out the same in both: all of them are held exactly.

    PYTHONPATH=TREE python tests/test_soft_outputs_gpu.py --record OUT.json      (TREE: a built checkout to record)
    python tests/test_soft_outputs_gpu.py --merge A.json B.json tests/golden/soft_outputs.json

Contexts: tests.tables.params_for(table, 1024, carriers, P=2, D=9) -- D = 9 is no multiple of the 8 symbol phases -- for
C = 70 (descending bins: one partial 64-wide column, one partial 256-tile) and C = 300 (ascending: a strided second pass of
the 256-thread loops, five columns for the two halves of noise_estimate_cs), on one table per arm of the table dispatch:
qpsk_ref (separable, its first label bit on the Q axis: the per-axis scan, HI 0), square 16-QAM (HI 2), qam64 (HI 3), psk8
(literal scan), rect8 (separable, not square); and on the two widest labels of tests/tables.py, ring8_mu7 (mu = 7, literal
scan) and grid16_mu8 (mu = 8, separable), whose digests were recorded on the commit that added them (its kernels are the
parent's).
Packets: F = 3 and, where F enters the launch geometry, the smallest F at which the symbols-per-workgroup rule
(nchunk = ceil(8 n_cu / per) clamped to [1, D], Dc = ceil(D / nchunk)) gives a Dc >= 2 that does not divide D: computed
from the engine's n_cu, asserted in the test.
Inputs are built on the host from np.random.RandomState and uploaded: table points plus noise at 15 dB, and
  packet 0: one NaN symbol, one symbol with an infinite part;
  packet 1: a NaN, a +Inf and a 0.0 carrier variance, a NaN symbol variance;
  packet 2: exact table points and variances all 0 (a flat packet);
  combining: in branch min(1, B - 1) a NaN channel estimate / an infinite variance on one carrier and an infinite symbol.
The fused sample-to-LLR call runs on rows of tables.demod_case with soft_kind 1, 3 and 0 (a scan table and a separable
one), on a square 16-QAM case built the same way (soft_kind 2: no row of tables.CASES has one) and on
test_fused_llr_gpu._extra_case's direct-store geometry."""
import functools
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soft_outputs.json")
N, P, D = 1024, 2, 9
SNR_DB = 15.0
CONTEXTS = [(t, C) for t in ("qpsk_ref", "qam16", "qam64", "psk8", "rect8", "ring8_mu7", "grid16_mu8") for C in (70, 300)]
SQUARE = ("qpsk_ref", "qam16", "qam64")
FUSED = {"qpsk_ref-contig-1024-P2-D3-float64": 1, "qam64-contig-1024-P2-D3-float64": 3,
         "psk8-all_reversed-1024-P1-D5-float64": 0, "rect8-comb2-1024-P2-D3-float64": 0,
         "ring8_mu7-all_reversed-1024-P1-D3-float64": 0, "grid16_mu8-shuffled-1024-P2-D3-float64": 0}
LEFT_OUT = []                                   # "case/item" that the parent's two recordings disagreed on: not in the golden file
CASES = [f"{t}-C{C}" for t, C in CONTEXTS] + ["fused-" + k for k in FUSED] + ["fused-qam16", "fused-direct-stores"]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def table_of(name):
    from oracle import gf3_oracle as orc
    from tests import tables as T
    return orc.square_qam_table(4) if name == "qam16" else T.TABLES[name]


def bins_of(C):
    return np.arange(20 + C - 1, 19, -1) if C == 70 else np.arange(20, 20 + C)


def symbols_per_group(n_cu, per, D):
    """The library's rule: about 8 workgroups per compute unit, `per` of them per data symbol chunk."""
    nchunk = min(max(-(-8 * n_cu // per), 1), D)
    return -(-D // nchunk)


def large_F(n_cu, ntile=1):
    """Smallest F > 3 whose Dc is at least 2 and does not divide D (a last workgroup with fewer symbols)."""
    for F in range(4, 8 * n_cu + 1):
        Dc = symbols_per_group(n_cu, F * ntile, D)
        if Dc >= 2 and D % Dc:
            return F, Dc
    raise AssertionError("no such F")


def order_of(C):
    """A 6/4/2/0 table in runs whose ends fall inside a wave."""
    ends = (20, 37, 59) if C == 70 else (90, 170, 250)
    order = np.zeros(C, dtype=np.uint8)
    order[:ends[0]], order[ends[0]:ends[1]], order[ends[1]:ends[2]] = 6, 4, 2
    assert all(e % 64 for e in ends)
    return order


def inputs(table, C, F, branches):
    """Host arrays of one (table, C, F): eq [F, D, C], variances, channel estimates and, for combining, four branches."""
    rs = np.random.RandomState(zlib.crc32(f"{table}-{C}-{F}".encode()))
    pts = np.asarray(table_of(table)[0], dtype=np.complex128)
    K = N // 2 - 1
    sigma = np.sqrt(np.mean(np.abs(pts) ** 2) / 10.0 ** (SNR_DB / 10.0) / 2.0)
    clean = pts[rs.randint(0, len(pts), (F, D, C))]
    noise = sigma * (rs.randn(F, D, C) + 1j * rs.randn(F, D, C))
    noise[2] = 0.0                                                  # packet 2: exact table points
    eq = clean + noise
    eq[0, 1, 5] = complex(np.nan, eq[0, 1, 5].imag)
    eq[0, 2, 7] = complex(eq[0, 2, 7].real, np.inf)
    var_c = 2.0 * sigma ** 2 * (0.25 + 1.5 * rs.rand(F, C))
    var_s = 2.0 * sigma ** 2 * (0.25 + 1.5 * rs.rand(F, D))
    var_c[1, 3], var_c[1, 4], var_c[1, 5], var_s[1, 2] = np.nan, np.inf, 0.0, np.nan
    var_c[1, 6] = 1e-9 * sigma ** 2                                 # under the floor of 1e-6 vbar
    var_c[2], var_s[2] = 0.0, 0.0
    Hs = rs.randn(F, K) + 1j * rs.randn(F, K)
    He = Hs * (1.0 + 0.2 * rs.randn(F, K)) + 0.1j * rs.randn(F, K)
    x = dict(eq=eq, var_c=var_c, var_s=var_s, Hs=Hs, He=He)
    if not branches:
        return x
    bins = bins_of(C)
    for b in range(4):                                              # the branches of one transmission
        e = clean + np.roll(noise, 97 * (b + 1), axis=2) * (1.0 + 0.5 * b)
        v = var_c * (1.0 + 0.5 * b)
        hs, he = np.roll(Hs, b + 1, axis=1).copy(), np.roll(He, b + 1, axis=1).copy()
        x[f"eq{b}"], x[f"var{b}"], x[f"Hs{b}"], x[f"He{b}"] = e, v, hs, he
    for B in (1, 2, 3, 4):                                          # what branch min(1, B - 1) holds when B branches are combined
        b = min(1, B - 1)
        e, v, hs = x[f"eq{b}"].copy(), x[f"var{b}"].copy(), x[f"Hs{b}"].copy()
        e[0, 3, 9] = complex(np.inf, 0.0)
        v[0, 2] = np.inf
        hs[0, bins[2] - 1] = complex(np.nan, 0.0)
        x[f"eq{b}/B{B}"], x[f"var{b}/B{B}"], x[f"Hs{b}/B{B}"] = e, v, hs
    return x


class Recorder:
    """item -> [digest of the named inputs' digests, digest of the output]."""

    def __init__(self, arrays):
        self.din = {k: sha(v) for k, v in arrays.items()}
        self.items = {}

    def put(self, item, used, out):
        key = hashlib.sha256(" ".join(self.din[k] for k in used).encode()).hexdigest()
        self.items[item] = [key, sha(out.cpu().numpy())]


def run_context(table, C):
    import torch
    from tests import tables as T
    from tests.util import engine_for
    p = T.params_for(table_of(table), N, bins_of(C), P=P, D=D)
    eng = engine_for(p)
    ntile = -(-C // 256)
    (F_big, Dc_big), (F_cmb, Dc_cmb) = large_F(eng.n_cu), large_F(eng.n_cu, ntile)
    assert Dc_big >= 2 and D % Dc_big and Dc_cmb >= 2 and D % Dc_cmb
    assert symbols_per_group(eng.n_cu, F_big, D) == Dc_big and symbols_per_group(eng.n_cu, F_cmb * ntile, D) == Dc_cmb
    items = {}
    # (tag, F, the single-branch calls, combining): with one 256-carrier tile the two large F are the same number
    passes = [("F3", 3, True, True), ("Fbig", F_big, True, ntile == 1)] + ([("Fcmb", F_cmb, False, True)] if ntile > 1 else [])
    for tag, F, single, combine in passes:
        x = inputs(table, C, F, combine)
        rec = Recorder(x)
        d = {k: torch.from_numpy(v).cuda() for k, v in x.items()}
        eq = d["eq"].reshape(F * D, C)
        if single:
            rec.put("soft_demap_csi", ("eq", "Hs", "He"), eng.soft_demap_csi(eq, d["Hs"], d["He"]))
            rec.put("soft_demap_nw", ("eq", "var_c"), eng.soft_demap_nw(eq, d["var_c"]))
            for de in (False, True):
                rec.put(f"soft_demap_nw2/deint{int(de)}", ("eq", "var_c", "var_s"),
                        eng.soft_demap_nw2(eq, d["var_c"], d["var_s"], deinterleave=de))
            if table in SQUARE:
                ld = eng.loading(order_of(C))
                rec.put("soft_demap_loaded/var", ("eq", "var_c"), eng.soft_demap_loaded(eq, ld, var=d["var_c"]))
                rec.put("soft_demap_loaded/csi", ("eq", "Hs", "He"), eng.soft_demap_loaded(eq, ld, Hs=d["Hs"], He=d["He"]))
                rec.put("soft_demap_loaded/unit", ("eq",), eng.soft_demap_loaded(eq, ld))
        if tag == "F3":
            rec.put("soft_demap", ("eq",), eng.soft_demap(eq, 0.7))
            rec.put("noise_estimate", ("eq",), eng.noise_estimate(eq))
            vc, vs = eng.noise_estimate2(eq)
            rec.put("noise_estimate2/var_c", ("eq",), vc)
            rec.put("noise_estimate2/var_s", ("eq",), vs)
            out, phase, measured = eng.track_phase(eq, want_track=True)
            for k, v in (("out", out), ("phase", phase), ("measured", measured)):
                rec.put(f"track_phase/{k}", ("eq",), v)
            if table in SQUARE:
                rec.put("noise_estimate_loaded", ("eq",), eng.noise_estimate_loaded(eq, eng.loading(order_of(C))))
        if combine:
            for B in (1, 2, 3, 4):
                names = {k: [f"{k}{b}/B{B}" if b == min(1, B - 1) and k != "He" else f"{k}{b}" for b in range(B)]
                         for k in ("eq", "var", "Hs", "He")}
                eqs = [d[k].reshape(F * D, C) for k in names["eq"]]
                for mode, kw, used in (("csi", dict(Hs=[d[k] for k in names["Hs"]], He=[d[k] for k in names["He"]]),
                                        names["eq"] + names["Hs"] + names["He"]),
                                       ("noise", dict(var=[d[k] for k in names["var"]]), names["eq"] + names["var"])):
                    o = eng.combine_branches(eqs, want=("eq", "w", "llr"), **kw)
                    for k in ("eq", "w", "llr"):
                        rec.put(f"combine_branches/B{B}/{mode}/{k}", used, o[k])
        items.update({f"{tag}/{k}": v for k, v in rec.items.items()})
        del d
    eng.close()
    return items


@functools.lru_cache(maxsize=None)
def fused_qam16_case():
    """Square 16-QAM (soft_kind 2) on the control map of N = 1024, built as tables.demod_case builds."""
    from oracle import gf3_oracle as orc
    from tests import tables as T
    p = T.params_for(orc.square_qam_table(4), 1024, T.contig(511), P=2, D=3)
    rs = np.random.RandomState(416)
    F = 2
    payload = T.existing_labels_payload(rs, p, F * p.D * p.C)
    gaps = rs.randint(0, 200, F)
    r = orc.tx_stream(payload, rs.choice(T.QPSK_FILL, size=p.K - p.C), p, gaps=gaps, lead=30, tail=60)
    r = np.convolve(r, T.ECHO)[: len(r)]
    r = r + T.NOISE_REL * np.sqrt(np.mean(r * r)) * rs.randn(len(r))
    starts = 30 + np.cumsum(gaps) + np.arange(F) * p.frame_len + p.Lc
    return p, r, starts


def run_fused(name):
    import torch
    from tests import tables as T
    from tests.test_fused_llr_gpu import _extra_case
    from tests.util import engine_for
    if name == "qam16":
        p, x, starts = fused_qam16_case()
    elif name == "direct-stores":
        p, x, starts, _ = _extra_case()
    else:
        p, x, starts, _, _ = T.demod_case(T.CASE_IDS.index(name))
    eng = engine_for(p)
    rec = Recorder({"x": x, "starts": np.asarray(starts, dtype=np.int64)})
    xd = torch.from_numpy(x).cuda()
    for w in ("csi", "none"):
        for split in (False, True):
            rec.put(f"demod_frames_llr/{w}/split{int(split)}", ("x", "starts"),
                    eng.demod_frames_llr(xd, starts, weight=w, split=split)["llr"])
    eng.close()
    return rec.items


def run(case):
    if case.startswith("fused-"):
        return run_fused(case[len("fused-"):])
    table, C = case.rsplit("-C", 1)
    return run_context(table, int(C))


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
