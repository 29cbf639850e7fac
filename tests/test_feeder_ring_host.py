"""The feeder's ring as warpdemux_amd/csrc/wdx_feeder_ring.h states it -- the layout of a slot's data regions and the
transitions of a slot's state word -- without a GPU and without processes: tests/host/feeder_ring_check.cpp is built with the
system C++ compiler and run.  Its `layout` answers over a grid of geometries are compared with the layout as restated here
(the ring format WDF3, byte for byte what wdx_feeder_ring_init has always written); the program itself asserts that the
regions tile the ring and writes every piece of every slot of the rings small enough to allocate, under the address and
undefined-behaviour sanitizers.  `script` walks the transitions in one thread, `stress` runs them between seven threads under
the thread sanitizer."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "feeder_ring_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC]
REGIONS = ("sig", "row_off", "row_len", "a_start", "a_end", "ok", "dist", "call", "status", "fpt", "dwell", "stats", "prob",
           "pred", "conf", "ridx")
# The header area in front of the regions: the ring's record (32 slot records of 264 bytes and the geometry, 8.6 KB) rounded
# up to pages; a refine ring keeps rp and the query (96 doubles) behind the record, which fits the same three pages.
HEADER_PLAIN, HEADER_REFINE = 12288, 12288


def _build(tmp_path, name, sanitize):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, *FLAGS, "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-pthread", SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("feeder_ring"), "feeder_ring_check", "address,undefined")


def _grid():
    return list(itertools.product((1, 2, 32), (1, 7, 1000), (1, 5, 4096, 10000), (0, 1, 4, 1368), (0, 25, 110), (0, 4, 16),
                                  (0, 1), (0, 1)))


def _up(v, a=4096):
    return (v + a - 1) // a * a


def _layout(n_slots, mr, stride, n_refs, K, kc, int16, refine):
    """ring_bytes, header bytes, the sixteen offsets and the sixteen per-slot strides"""
    sig_floats = mr * ((stride + 7) // 8 * 8 + 8) // 2 if int16 else mr * ((stride + 3) // 4 * 4 + 4)
    sig_floats = max(sig_floats, K * 2 * mr)
    i32 = _up(mr * 4)
    fpt = _up(mr * K * 8) if K else 0
    strides = [_up(sig_floats * 4 + (mr * 12 if int16 else 0)), _up((mr + 1) * 8), i32, i32, i32, _up(mr),
               _up(mr * (n_refs or 1) * 4), i32, i32, fpt, fpt, _up(mr * 48) if K else 0, _up(mr * kc * 8) if kc else 0,
               i32 if kc else 0, _up(mr * 8) if kc else 0, _up(mr * 12) if refine else 0]
    header = HEADER_REFINE if refine else HEADER_PLAIN
    offs, o = [], header
    for s in strides:
        offs.append(o)
        o += n_slots * s
    return [o, header] + offs + strides


def test_ring_layout_over_the_geometry_grid_under_sanitizers(checked):
    grid = _grid()
    assert len(grid) == 3 * 3 * 4 * 4 * 3 * 3 * 2 * 2
    text = "".join(" ".join(map(str, g)) + "\n" for g in grid)
    run = subprocess.run([checked, "layout"], input=text.encode(), capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    tail = run.stderr.decode().strip().splitlines()[-1].split()
    assert int(tail[0]) == len(grid), run.stderr[-2000:]
    assert int(tail[2]) > len(grid) // 4, "too few rings were small enough to be written"
    got = [list(map(int, line.split())) for line in run.stdout.decode().splitlines()]
    assert len(got) == len(grid)
    for g, have in zip(grid, got):
        want = _layout(*g)
        assert have == want, (g, [(n, h, w) for n, h, w in zip(("bytes", "header") + REGIONS + REGIONS, have, want) if h != w])


def test_slot_transitions_scripted_under_sanitizers(checked):
    run = subprocess.run([checked, "script"], capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr.decode().strip().endswith("script ok")


def test_slot_transitions_under_contention_under_the_thread_sanitizer(tmp_path):
    exe = _build(tmp_path, "feeder_ring_tsan", "thread")
    run = subprocess.run([exe, "stress", "8000"], capture_output=True)
    err = run.stderr.decode()
    assert run.returncode == 0 and "ThreadSanitizer" not in err, err[-4000:]
    words = err.strip().splitlines()[-1].replace(",", "").split()
    served, disowned, wrong = (int(words[words.index(k) + 1]) for k in ("served", "disowned", "wrong"))
    assert wrong == 0 and served == 6 * 8000 + disowned, err[-2000:]
