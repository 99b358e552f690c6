"""The guard-band harness (tests/guarded.py) is not vacuous, and no ABI entry is silently left out of it.

On CPU tensors a stand-in "call" commits each fault the harness exists for -- a byte written in front of a view, a byte
written behind it, a promised element left unwritten, an input changed, an element from outside an input let into an
output -- and every one is reported with the array's name and the byte offset.  A well-behaved stand-in passes, at both
skews.  The census at the end holds every name of `_lib._SIGS` to be a row of a case table, a key of EXEMPT, or one of the
entries listed in WITHHELD as still owed a row: a new ABI entry fails it until it has a case."""
import collections
import ctypes
import glob
import importlib
import os

import numpy as np
import pytest
import torch

from tests import guarded as G

N = 37                                                              # odd: the skewed view ends off every power of two


def _poke(view, byte_offset, value=0x11):
    """Write one byte at an offset from the view's first byte, as a kernel with a wrong index would."""
    (ctypes.c_uint8 * 1).from_address(view.data_ptr() + byte_offset)[0] = value


def _peek_f64(view, element):
    return (ctypes.c_double * 1).from_address(view.data_ptr() + 8 * element)[0]


def standin(fault=None):
    """out[i] = 2 x[i] + k[i] (k int16 'samples'), status[0] stays (documented not written); `fault` breaks it one way."""
    def call(a):
        x = a.in_("d_x", np.arange(N, dtype=np.float64) + 0.5)
        k = a.in_("d_k", np.arange(N, dtype=np.int16), samples=True)
        out = a.out("d_out", (N,), torch.float64)
        st = a.inout("d_status", np.array([7, 7], dtype=np.int32))
        a.work("d_work", 24)
        out.copy_(2 * x + k.to(torch.float64))
        st[1] = 3
        a.keep("d_status", np.s_[:1])
        a.result("rc", 0)
        if fault == "before":
            _poke(out, -1)
        elif fault == "after":
            _poke(out, 8 * N)
        elif fault == "work_after":
            _poke(a.items["d_work"]["view"], 24)
        elif fault == "unwritten":
            for i in range(8):                                       # the pre-fill, put back
                _poke(out, 8 * 5 + i, G._FILL[a.dressing])
        elif fault == "input":
            _poke(x, 8 * 3 + 2)
        elif fault == "kept":
            st[0] = 9
        elif fault == "read_outside" and a.dressing is not None:     # (a plain tensor has nothing the stand-in may read there)
            out[N - 1] = 2 * x[N - 1] + _peek_f64(x, N)
        elif fault == "sample_outside" and a.dressing is not None:
            k_before = (ctypes.c_int16 * 1).from_address(k.data_ptr() - 2)[0]
            out[1] = out[1] + float(k_before)                        # an integer has no NaN: the extremes of opposite sign show it
    return call


@pytest.mark.parametrize("skew", [False, True])
def test_a_well_behaved_call_passes(skew):
    plain = G.run(standin(), skews=(skew,))
    assert plain.items["d_out"]["view"].tolist() == [2 * (i + 0.5) + i for i in range(N)]


def test_views_are_where_the_rule_puts_them():
    for skew in (False, True):
        a = G.Arrays("A", skew)
        c = a.in_("c", np.zeros(3, dtype=np.complex128))
        b = a.out("b", (5,), torch.uint8)
        m = a.out("m", (16,), torch.uint8, align=8)
        s = a.in_("s", np.zeros(4, dtype=np.int16), samples=True)
        w = a.work("w", 24)                                          # a workspace is never skewed below what is carved out of it
        for v, step, name in ((c, 16, "c"), (b, 1, "b"), (m, 8, "m"), (s, 2, "s"), (w, G.WORK_ALIGN, "w")):
            it = a.items[name]
            assert it["lo"] == G.GUARD + (step if skew else 0) and it["whole"].numel() == it["lo"] + it["nbytes"] + G.GUARD
            assert v.is_contiguous() and v.data_ptr() == it["whole"].data_ptr() + it["lo"]
        assert m.data_ptr() % 8 == 0 and c.data_ptr() % 8 == 0
        assert a.items["s"]["whole"].view(torch.int16)[0] == 32767 and a.items["s"]["whole"].view(torch.int16)[-1] == 32767
        assert torch.isnan(a.items["c"]["whole"][: G.GUARD].view(torch.float64)).all() and (b == 0xFF).all()
    z = G.Arrays("B", True)
    assert z.in_("s", np.zeros(4, dtype=np.int16), samples=True).tolist() == [0] * 4
    assert z.items["s"]["whole"].view(torch.int16)[0] == -32768 and (z.out("b", (5,), torch.uint8) == 0x5A).all()
    assert (z.items["b"]["whole"][: G.GUARD] == 0).all()


@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("fault, text", [
    ("before", r"d_out: band byte at offset -1 "),
    ("after", rf"d_out: band byte at offset {8 * N} "),
    ("work_after", r"d_work: band byte at offset 24 "),
    ("unwritten", r"d_out: byte at offset 40 \(element 5\) differs"),
    ("input", r"d_x: input byte at offset 26 was changed"),
    ("kept", r"d_status: byte at offset 0 lies in a range the header says is not written"),
    ("read_outside", rf"d_out: byte at offset {8 * (N - 1)}"),
    ("sample_outside", r"d_out: byte at offset (8|9|1[0-5]) \(element 1\) differs"),
])
def test_every_fault_is_reported_with_array_and_offset(fault, text, skew):
    with pytest.raises(G.Violation, match=text):
        G.run(standin(fault), skews=(skew,))


def test_a_result_that_depends_on_the_dressing_is_reported():
    def call(a):
        a.result("count", 1 if a.dressing == "A" else 2)
    with pytest.raises(G.Violation, match="host results differ"):
        G.run(call)


# ---- the census -------------------------------------------------------------------------------------------------------------
NO_DEVICE_MEMORY = "launches no kernel and touches no caller device memory"
HOST_ONLY = "writes host memory only"
EXEMPT = {name: NO_DEVICE_MEMORY for name in (
    "gf3_version", "gf3_source_hash", "gf3_ctx_create", "gf3_ctx_destroy", "gf3_last_error", "gf3_clear_runtime_error",
    "gf3_debug_set_stamps", "gf3_bytes_per_frame", "gf3_sync_max_window", "gf3_sync_stream_workspace_bytes",
    "gf3_demod_workspace_bytes", "gf3_demod_split_plan", "gf3_demod_frames_last", "gf3_demod_screen_workspace_bytes",
    "gf3_sync_frames_workspace_bytes", "gf3_sync_frames_last", "gf3_sync_chunk_workspace_bytes",
    "gf3_sync_decide_workspace_bytes", "gf3_detect_chunk_workspace_bytes", "gf3_sync_stream_mode", "gf3_sync_stream_info",
    "gf3_known_h_workspace_bytes", "gf3_loading_create", "gf3_loading_destroy", "gf3_loading_bits",
    "gf3_feedback_workspace_bytes", "gf3_ldpc_create", "gf3_ldpc_destroy", "gf3_ldpc_n", "gf3_ldpc_k")}
EXEMPT.update({"gf3_chirp_replica": HOST_ONLY, "gf3_resample_coefficients": HOST_ONLY})
# Entries that are owed a row and have none.  Not exemptions: a name leaves this list only by gaining a row, and the census
# below refuses a name that is in it and in a table, or in it and not in `_SIGS`.
#   FAULTED: a guarded call of gf3_sync_stream whose workspace sat one byte off its alignment ended in a GPU memory fault
#     (the kernels read the int64 words kept in `d_work` as aligned words).  The harness never under-aligns a
#     workspace any more (guarded.WORK_ALIGN, and gf3rx.h now demands it); the rows of the entries that launch spec_kernel,
#     ols_kernel, pk_scan or pk_nms, or need their output, wait until that reading of the fault is confirmed.
#   NO_ROW: no guarded case has been written and seen to pass for the entry yet.
FAULTED = "a guarded call of its kernels faulted on the GPU with a workspace off its alignment; reading not confirmed"
NO_ROW = "no guarded case yet"
WITHHELD = {name: FAULTED for name in ("gf3_sync_stream", "gf3_sync_stream_ex", "gf3_sync_chunk", "gf3_sync_decide",
                                       "gf3_detect_chunk", "gf3_detect_decide")}
WITHHELD.update({name: NO_ROW for name in ("gf3_debug_stream_screen",)})      # (with the stream-sync family: its rows wait)


def bounds_modules():
    """Every tests/test_bounds_*_gpu.py, imported in sorted order: the siblings enter their rows in the two tables on import."""
    here = os.path.dirname(os.path.abspath(__file__))
    names = sorted(os.path.basename(f)[:-3] for f in glob.glob(os.path.join(here, "test_bounds_*_gpu.py")))
    return {name: importlib.import_module("tests." + name) for name in names}


def test_every_abi_entry_has_a_case_or_an_accepted_exemption():
    from gf3_audio_modem_amd import _lib
    mods = bounds_modules()
    BC, BS = mods["test_bounds_coding_gpu"], mods["test_bounds_signal_gpu"]
    rows = set(BS.CASES) | set(BC.CASES)
    assert not set(BS.CASES) & set(BC.CASES)
    assert set(EXEMPT.values()) == {NO_DEVICE_MEMORY, HOST_ONLY}
    assert not rows & set(EXEMPT), sorted(rows & set(EXEMPT))
    assert not (rows | set(EXEMPT)) & set(WITHHELD)                                   # (a name leaves WITHHELD by gaining a row)
    missing = set(_lib._SIGS) - rows - set(EXEMPT) - set(WITHHELD)
    assert not missing, f"ABI entries with neither a guarded case nor an exemption: {sorted(missing)}"
    known = rows | set(EXEMPT) | set(WITHHELD)
    assert not known - set(_lib._SIGS), sorted(known - set(_lib._SIGS))
    for name, cases in {**BS.CASES, **BC.CASES}.items():
        assert cases, name


def test_every_registered_row_is_run_by_exactly_one_module():
    """A sibling module enters rows with `BS.case` and runs the names of its own ENTRIES: a name registered and left out of
    ENTRIES would satisfy the census above and never run.  The union of the modules' ROWS is every (name, i) of both tables,
    and no pair is in two modules."""
    mods = bounds_modules()
    BC, BS = mods["test_bounds_coding_gpu"], mods["test_bounds_signal_gpu"]
    registered = {(name, i) for table in (BS.CASES, BC.CASES) for name, cases in table.items() for i in range(len(cases))}
    run = collections.Counter(pair for m in mods.values() for pair in m.ROWS)
    twice = sorted(pair for pair, n in run.items() if n > 1)
    assert not twice, f"rows run by two modules: {twice[:5]}"
    assert set(run) == registered, (sorted(registered - set(run))[:5], sorted(set(run) - registered)[:5])
    assert WITHHELD["gf3_debug_stream_screen"] == NO_ROW and sum(v == FAULTED for v in WITHHELD.values()) == 6
