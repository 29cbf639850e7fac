"""The layout of a caller's d_work and the four *_workspace_bytes functions, without a GPU:
warpdemux_amd/csrc/wdx_work_layout.h swept by tests/host/work_layout_check.cpp -- built with the system C++ compiler under the
address and undefined-behaviour sanitizers (stand-alone: nothing is preloaded).  The program itself asserts, point by point,
that no two pieces overlap, that every piece ends inside the promised size, the alignments, and that a slice of a shard never
needs more than the whole call was promised; here the Python restatement the GPU tests read the counters by
(tests/helpers/framed.py: work_pieces) is pinned against the header, and the library's own size functions against both."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import framed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "work_layout_check.cpp")
POINTS = [(n, K) for n in (0, 1, 63, 64, 65, 300, 2304, 8191, 8192, 8193, 20000) for K in (1, 13, 25, 110, 128)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    out = str(tmp_path_factory.mktemp("work_layout") / "work_layout_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", out])
    return out


def test_layout_over_its_domain_under_sanitizers(exe):
    run = subprocess.run([exe], capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    words = run.stderr.decode().split()
    assert words[-1] == "points" and int(words[-2]) > 3_000_000, run.stderr[-200:]


def test_python_restatement_is_the_headers(exe):
    for n, K in POINTS:
        got = [int(v) for v in subprocess.run([exe, str(n), str(K)], capture_output=True, check=True).stdout.split()]
        w = framed.work_pieces(n, K)
        want = [w["fp_ws"], w["count"], w["clip"], *w["lists"], w["split"], w["dbg"], w["fp_bytes"], w["plain_bytes"],
                w["refine_off"], w["refine_bytes"]]
        assert got == want, (n, K)
    assert framed.N_COUNTERS == len(framed.COUNTER_NAMES) == 8


def test_library_size_functions_are_the_headers():
    """wdx_demux_workspace_bytes / wdx_demux_refine_workspace_bytes return what the header states (no GPU: they take no context)"""
    from warpdemux_amd import _lib

    L = _lib.load()
    for n, K in POINTS:
        w = framed.work_pieces(n, K)
        assert L.wdx_demux_workspace_bytes(n, K) == w["plain_bytes"], (n, K)
        assert L.wdx_demux_refine_workspace_bytes(n, K) == w["refine_bytes"], (n, K)
    # the statement of tests/test_refine_paths_host.py, unchanged: the plain size to 256, plus 1 632 bytes per read
    sizes = np.array([[L.wdx_demux_workspace_bytes(n, 25), L.wdx_demux_refine_workspace_bytes(n, 25)] for n in (1, 96, 8192)])
    assert (sizes[:, 1] == (sizes[:, 0] + 255) // 256 * 256 + 1632 * np.array([1, 96, 8192])).all()
    assert L.wdx_demux_workspace_bytes(-1, 25) == 0 and L.wdx_demux_workspace_bytes(4, 0) == 0
    assert L.wdx_demux_refine_workspace_bytes(-1, 25) == 0
