"""The host-side pieces of the coded chain (gf3_audio_modem_amd/coding.py, outer.py) that need neither a GPU nor the
library: the named small copy, the outer code's strided placement pair, and the decode report."""
import numpy as np
import pytest
import torch

from gf3_audio_modem_amd.coding import decode_report, fetch
from gf3_audio_modem_amd.outer import from_transmitted, to_transmitted, transmitted_index


def test_fetch_round_trip_on_cpu_tensors():
    rng = np.random.default_rng(11)
    src = {"Hs0": rng.normal(size=7) + 1j * rng.normal(size=7),                    # complex128 [K]
           "slope": np.array([0.25, -1e-300, np.inf, -np.inf, np.nan]),             # float64 [F], non-finite included
           "iters": np.array([3, -50, 1, -2147483648, 2147483647], dtype=np.int32),
           "status": np.zeros(0, dtype=np.int32),                                   # (the status without an outer code)
           "ragged": np.array([1], dtype=np.int32),
           "snr": rng.normal(size=(2, 3))}                                          # a shape to restore
    src["Hs0"][2] = complex(np.nan, -np.inf)
    got = fetch({k: torch.from_numpy(v) for k, v in src.items()})
    assert list(got) == list(src)                                                   # names, in order
    for k, v in src.items():
        assert got[k].shape == v.shape and got[k].dtype == v.dtype, k
        assert np.array_equal(got[k].view(np.uint8), v.view(np.uint8)), k           # bit for bit (NaN, signed infinities)
    arrays = list(got.values())
    for i, a in enumerate(arrays):
        for b in arrays[i + 1:]:
            assert not np.shares_memory(a, b)
    got["iters"][:] = 0                                                             # writable, and nobody else's memory
    assert got["ragged"][0] == 1 and got["slope"][0] == 0.25


@pytest.mark.parametrize("G,R,NG", [(1, 1, 1), (4, 2, 1), (4, 2, 4), (20, 4, 13)])
def test_strided_placement_pair(G, R, NG):
    k = 8
    g, t = np.meshgrid(np.arange(NG), np.arange(G + R), indexing="ij")
    members = np.broadcast_to((g * 1000 + t)[:, :, None], (NG, G + R, k)).astype(np.int64)      # contents name (g, t)
    members = members + np.arange(k) * 100_000
    data, parity = torch.from_numpy(members[:, :G].copy()), torch.from_numpy(members[:, G:].copy())
    sent = to_transmitted(data, parity)
    assert tuple(sent.shape) == ((G + R) * NG, k)
    for gi in range(NG):
        for ti in range(G + R):
            assert np.array_equal(sent[transmitted_index(gi, ti, NG)].numpy(), members[gi, ti]), (gi, ti)
    back = from_transmitted(sent, NG, G)
    assert tuple(back.shape) == (NG * G, k) and np.array_equal(back.numpy(), members[:, :G].reshape(NG * G, k))


def test_report_counts_the_fill_without_statuses_and_only_the_groups_with_them():
    # 18 members of NG = 3 groups of (4, 2), then 3 rows of fill that "failed"
    iters = np.array([1, 2, -50, 1, 1, 3, 1, -50, 1, 1, 1, 1, -50, -50, -50, 1, 1, 1, -50, -50, -50], dtype=np.int32)
    rep = decode_report(iters, np.zeros(0, dtype=np.int32))
    assert {k: v for k, v in rep.items() if k != "failed_codewords"} == \
        {"codewords": 21, "inner_failed": 8, "recovered": 0, "groups_failed": 0}
    assert rep["failed_codewords"].tolist() == [2, 7, 12, 13, 14, 18, 19, 20] and rep["failed_codewords"].dtype == np.int64
    rep = decode_report(iters, np.array([2, 0, -3], dtype=np.int32), (4, 2))
    assert {k: v for k, v in rep.items() if k != "failed_codewords"} == \
        {"codewords": 18, "inner_failed": 5, "recovered": 2, "groups_failed": 1}
    assert rep["failed_codewords"].tolist() == [2, 7, 12, 13, 14]
    assert all(type(rep[k]) is int for k in ("codewords", "inner_failed", "recovered", "groups_failed"))
