"""Plain gf3_sync_frames from C (tests/c_client/gf3_sync_frames_client.c): no workspace, no mode argument -- the library
decides how the windows are evaluated and owns the memory that takes.  CPU: the program compiles and links.  GPU: it
returns the multipath fixture's offsets, by the screened path."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_c_client import LIBDIR, ROCM, ROOT, _write_case
from tests.util import load, params_of

SRC = os.path.join(ROOT, "tests", "c_client", "gf3_sync_frames_client.c")


def _build(out):
    from gf3_audio_modem_amd import build
    build.build_lib()
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    cmd = [cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROCM, "include"), SRC, "-o", out, "-L" + LIBDIR, "-lgf3rx", "-L" + os.path.join(ROCM, "lib"), "-lamdhip64",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_the_sync_frames_client_links(tmp_path):
    exe = _build(str(tmp_path / "gf3_sync_frames_client"))
    assert os.path.getsize(exe) > 0


@pytest.mark.gpu
def test_plain_sync_frames_from_c_returns_the_fixture_offsets(tmp_path):
    """g3 (echoes: several extrema above the threshold before the largest), one 400-lag window around every chirp but the
    last, one call each on the default stream: peak + 2 (what get_symbols hands the demodulator), every call screened."""
    exe = _build(str(tmp_path / "gf3_sync_frames_client"))
    g = load("g3_n4096_16qam_gr5")
    p = params_of(g)
    case, out = str(tmp_path / "g3.bin"), str(tmp_path / "g3.starts")
    _write_case(case, p, g["r"].astype("<f8"), 0, False)
    peaks = [int(pk) for pk in g["peaks"][:-1]]
    los = [pk + 1 - (p.Lc - 1) - 150 for pk in peaks]
    r = subprocess.run([exe, case, out, "400"] + [str(lo) for lo in los], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    raw = np.fromfile(out, dtype="<i8")
    assert raw[0] == len(raw) - 1 == 2 * len(peaks)
    starts, paths = raw[1::2], raw[2::2]
    assert np.array_equal(starts, np.array(peaks) + 2), (starts, peaks)
    assert np.all(paths == 0), paths                            # 0: the fp32 screen + fp64 on what it leaves open
