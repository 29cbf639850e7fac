"""The DTW dispatch rule (warpdemux_amd/csrc/wdx_dtw_plan.h: dtw_plan), without a GPU.

tests/host/dtw_plan_check.cpp is built with the system C++ compiler under the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded) and run as a child process.
(1) It prints the plan of every shape of PARENT_RECORDS below, and the plans must be those records.  The records are what the
dispatch did BEFORE the rule had one statement: the route census of DESIGN.md 4.3 (measured on an MI355X through
wdx_dtw_last_launch) and the edges tests/test_gpu_dtw_dispatch.py and tests/test_gpu_wide_dtw.py assert on the GPU, each
worked out from the arithmetic of the dispatcher as it stood then (launch_dtw, dtw_dev_route, demux_dev_rows) -- never from
dtw_plan.
(2) Over a sweep of 10.8 million shapes the program itself checks what must hold of every plan (the invariants are numbered in
its check()); the test asserts that none failed and that the sweep met every kernel family.
(3) The header stands alone and is a dependency of every object of the library."""
import os
import shutil
import subprocess

import pytest

from warpdemux_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "dtw_plan_check.cpp")

# One line per case: nX nY L window want_argmin entry(0 matrix entries, 1 fused device entries) no_wavefront no_short_dtw wide_dtw
#   | wdx_dtw_launch_info: family band_w exact_w layout fused_argmin launches refs_per_block window grid_x grid_y
#   | unsupported prep(0 none, 1 read-minor copy, 2 padded reads) ld copy_bytes flag_bytes argmin_after lds_bytes scratch_bytes
#     lanes rows
PARENT_RECORDS = """
65 5 200 15 1 0 0 0 0 1 0 0 0 0 1 1 15 21 1 0 0 0 0 0 1 51200 0 65 5
65 5 200 15 1 0 1 0 0 3 15 1 1 0 1 1 15 2 5 0 1 128 204800 128 1 0 0 65 5
70 9 110 5 1 0 0 0 0 1 0 0 0 0 1 1 5 40 1 0 0 0 0 0 1 28160 0 70 9
70 9 110 5 1 0 1 0 0 3 8 0 1 0 1 1 5 2 9 0 1 128 112640 128 1 0 0 70 9
70 9 110 16 1 0 0 0 0 1 0 0 0 0 1 1 16 40 1 0 0 0 0 0 1 28160 0 70 9
70 9 110 16 1 0 1 0 0 3 16 0 1 0 1 1 16 2 9 0 1 128 112640 128 1 0 0 70 9
70 9 110 17 1 0 0 0 0 3 32 0 1 0 1 1 17 2 9 0 1 128 112640 128 1 0 0 70 9
70 9 25 0 1 0 0 0 0 3 32 0 1 0 1 1 25 2 9 0 1 128 25600 128 1 0 0 70 9
70 9 110 33 1 0 0 0 0 4 0 0 1 0 1 9 33 2 1 0 1 128 112640 128 1 0 116391936 70 9
130 10 110 15 1 0 0 0 0 1 0 0 0 0 1 1 15 82 1 0 0 0 0 0 1 28160 0 130 10
130 10 110 15 1 0 1 0 0 3 15 1 1 0 1 1 15 3 10 0 1 192 168960 192 1 0 0 130 10
300 851 25 15 1 0 0 0 0 2 15 1 1 0 1 3 15 5 284 0 1 320 64000 320 1 0 0 300 851
5000 10 110 15 1 0 0 0 0 3 15 1 1 0 1 1 15 79 10 0 1 5056 4449280 5056 1 0 0 5000 10
3 1368 25 15 1 0 0 0 0 1 0 0 0 0 1 1 15 257 1 0 0 0 0 0 1 6400 0 3 1368
3 1368 25 15 1 0 1 0 0 2 15 1 2 0 1 1 15 22 3 0 2 87 2088 64 1 0 0 1368 3
63 1368 25 15 1 0 0 0 0 2 15 1 2 0 1 1 15 22 63 0 2 87 43848 64 1 0 0 1368 63
65 1368 25 15 1 0 0 0 0 2 15 1 1 0 1 2 15 2 684 0 1 128 25600 128 1 0 0 65 1368
140000 10 110 15 1 0 0 0 0 3 15 1 0 1 1 10 15 2188 1 0 0 0 0 0 0 0 0 140000 10
3000 64 25 15 1 0 0 0 0 2 15 1 1 0 1 2 15 47 32 0 1 3008 601600 3008 1 0 0 3000 64
20000 64 110 15 1 0 0 0 0 3 15 1 0 0 1 10 15 313 7 0 0 0 0 0 1 0 0 20000 64
40000 10 110 15 1 0 0 0 0 3 15 1 0 0 1 3 15 625 4 0 0 0 0 0 1 0 0 40000 10
2000 10 25 15 1 0 0 0 0 2 15 1 1 0 1 1 15 32 10 0 1 2048 409600 2048 1 0 0 2000 10
1000000 10 110 0 1 0 0 0 1 6 0 0 0 1 1 10 110 15625 1 0 0 0 0 0 0 56320 0 1000000 10
4096 851 64 0 1 0 0 0 1 6 0 0 1 0 1 16 64 64 54 0 1 4096 2097152 4096 1 32768 0 4096 851
65536 9 110 33 0 0 0 0 0 4 0 0 1 0 1 9 33 1024 1 0 1 65536 57671680 65536 0 0 116391936 65536 9
65537 9 110 33 1 0 0 0 0 4 0 0 1 0 2 9 33 1 1 0 1 65600 57728000 65600 1 0 116391936 65537 9
131073 9 110 33 1 0 0 0 0 4 0 0 1 0 3 9 33 1 1 0 1 131136 115399680 131136 1 0 116391936 131073 9
131008 31 25 15 1 0 0 0 0 2 15 1 0 0 1 16 15 2047 2 0 0 0 0 0 1 0 0 131008 31
131009 31 25 15 1 0 0 0 0 2 15 1 0 1 1 31 15 2048 1 0 0 0 0 0 0 0 0 131009 31
131008 32 25 15 1 0 0 0 0 2 15 1 0 0 1 16 15 2047 2 0 0 0 0 0 1 0 0 131008 32
131009 32 25 15 1 0 0 0 0 2 15 1 0 0 1 16 15 2048 2 0 0 0 0 0 1 0 0 131009 32
131009 31 25 15 0 0 0 0 0 2 15 1 0 0 1 31 15 2048 1 0 0 0 0 0 0 0 0 131009 31
1572800 64 25 15 1 0 0 0 0 2 15 1 0 0 1 32 15 24575 2 0 0 0 0 0 1 0 0 1572800 64
1572864 64 25 15 1 0 0 0 0 2 15 1 0 1 1 64 15 24576 1 0 0 0 0 0 0 0 0 1572864 64
8191 10 25 15 1 0 0 0 0 2 15 1 1 0 1 1 15 128 10 0 1 8192 1638400 8192 1 0 0 8191 10
8192 10 25 15 1 0 0 0 0 2 15 1 0 0 1 1 15 128 10 0 0 0 0 0 1 0 0 8192 10
8191 10 110 15 1 0 0 1 0 3 15 1 1 0 1 1 15 128 10 0 1 8192 7208960 8192 1 0 0 8191 10
8192 10 110 15 1 0 0 1 0 3 15 1 0 0 1 1 15 128 10 0 0 0 0 0 1 0 0 8192 10
8192 10 110 33 1 0 0 0 0 4 0 0 1 0 1 10 33 128 1 0 1 8192 7208960 8192 1 0 116391936 8192 10
63 64 25 15 1 0 1 0 0 2 15 1 2 0 1 1 15 1 63 0 2 87 43848 64 1 0 0 64 63
64 65 25 15 1 0 1 0 0 2 15 1 1 0 1 1 15 1 65 0 1 64 12800 64 1 0 0 64 65
63 63 25 15 1 0 1 0 0 2 15 1 1 0 1 1 15 1 63 0 1 64 12800 64 1 0 0 63 63
1 1368 110 0 1 0 0 0 0 4 0 0 2 0 1 1 110 22 1 0 2 172 1376 64 1 0 116391936 1368 1
1 1368 110 0 1 0 0 0 1 6 0 0 2 0 1 1 110 22 1 0 2 172 1376 64 1 56320 0 1368 1
4096 4 110 16 1 0 0 0 0 1 0 0 0 0 1 1 16 1024 1 0 0 0 0 0 1 28160 0 4096 4
3277 5 110 16 1 0 0 0 0 3 16 0 1 0 1 1 16 52 5 0 1 3328 2928640 3328 1 0 0 3277 5
4096 4 110 17 0 0 0 0 0 3 32 0 1 0 1 1 17 64 4 0 1 4096 3604480 4096 0 0 0 4096 4
1 1 257 1 0 0 0 0 0 3 8 0 1 0 1 1 1 1 1 0 1 64 131584 64 0 0 0 1 1
10 3 25 15 1 1 0 0 0 2 15 1 1 0 1 1 15 1 3 0 1 64 12800 64 1 0 0 10 3
10 3 25 15 1 1 0 1 0 3 15 1 1 0 1 1 15 1 3 0 1 64 12800 64 1 0 0 10 3
10 3 110 5 1 1 0 0 0 3 8 0 1 0 1 1 5 1 3 0 1 64 56320 64 1 0 0 10 3
10 1368 25 15 1 1 0 0 0 2 15 1 1 0 1 1 15 1 1368 0 1 64 12800 64 1 0 0 10 1368
8192 3 25 15 1 1 0 0 0 2 15 1 0 0 1 1 15 128 3 0 0 0 0 0 1 0 0 8192 3
10 3 110 33 1 1 0 0 0 0 0 0 0 0 0 0 0 0 0 1 0 0 0 0 0 0 0 0 0
10 3 110 0 1 1 0 0 1 6 0 0 1 0 1 1 110 1 3 0 1 64 56320 64 1 56320 0 10 3
0 3 110 33 1 1 0 0 0 0 0 0 0 0 0 0 0 0 0 1 0 0 0 0 0 0 0 0 0
10 3 300 0 1 1 0 0 1 0 0 0 0 0 0 0 0 0 0 1 0 0 0 0 0 0 0 0 0
"""
FIELDS = ("family band_w exact_w layout fused_argmin launches refs_per_block window grid_x grid_y unsupported prep ld copy_bytes "
          "flag_bytes argmin_after lds_bytes scratch_bytes lanes rows").split()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    out = str(tmp_path_factory.mktemp("dtw_plan") / "dtw_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", out])
    return out


def _records():
    return [tuple(int(v) for v in ln.split()) for ln in PARENT_RECORDS.strip().splitlines()]


def test_plans_are_the_parent_dispatch_records(exe):
    want = _records()
    assert len(want) == 57 and all(len(r) == 9 + len(FIELDS) for r in want)
    cases = "".join(" ".join(map(str, r[:9])) + "\n" for r in want)
    run = subprocess.run([exe], input=cases.encode(), capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(int(v) for v in ln.split()) for ln in run.stdout.decode().splitlines()]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[:9] == w[:9]
        bad = {f: (a, b) for f, a, b in zip(FIELDS, g[9:], w[9:]) if a != b}
        assert not bad, "case %s: (plan, record) %s" % (w[:9], bad)


def test_records_cover_the_census_and_the_edges_the_gpu_tests_assert():
    """the list above holds the census of DESIGN.md 4.3 and the edges the GPU tests assert: a guard against a record dropped later"""
    rec = {r[:9]: dict(zip(FIELDS, r[9:])) for r in _records()}
    fam = lambda *c: _lib.DTW_FAMILY_NAMES[rec[c]["family"]]
    lay = lambda *c: _lib.DTW_LAYOUT_NAMES[rec[c]["layout"]]
    # census: family, layout, grid, refs per block, fused
    route = lambda *c: (fam(*c), rec[c]["band_w"], lay(*c), rec[c]["grid_x"], rec[c]["grid_y"], rec[c]["refs_per_block"],
                        rec[c]["fused_argmin"])
    assert route(65, 5, 200, 15, 1, 0, 0, 0, 0)[0] == "wavefront"
    assert route(65, 5, 200, 15, 1, 0, 1, 0, 0) == ("band", 15, "read-minor", 2, 5, 1, 0)
    assert route(70, 9, 110, 5, 1, 0, 1, 0, 0) == ("band", 8, "read-minor", 2, 9, 1, 0)
    assert route(70, 9, 110, 16, 1, 0, 1, 0, 0) == ("band", 16, "read-minor", 2, 9, 1, 0)
    assert route(70, 9, 110, 17, 1, 0, 0, 0, 0) == ("band", 32, "read-minor", 2, 9, 1, 0)
    assert route(70, 9, 25, 0, 1, 0, 0, 0, 0) == ("band", 32, "read-minor", 2, 9, 1, 0)
    assert (fam(70, 9, 110, 33, 1, 0, 0, 0, 0), rec[(70, 9, 110, 33, 1, 0, 0, 0, 0)]["launches"]) == ("scratch", 1)
    assert route(130, 10, 110, 15, 1, 0, 1, 0, 0) == ("band", 15, "read-minor", 3, 10, 1, 0)
    assert route(300, 851, 25, 15, 1, 0, 0, 0, 0) == ("short", 15, "read-minor", 5, 284, 3, 0)
    assert route(5000, 10, 110, 15, 1, 0, 0, 0, 0) == ("band", 15, "read-minor", 79, 10, 1, 0)
    assert route(3, 1368, 25, 15, 1, 0, 0, 0, 0)[0] == "wavefront"
    assert route(3, 1368, 25, 15, 1, 0, 1, 0, 0)[:5] == ("short", 15, "refs-as-lanes", 22, 3)
    assert route(63, 1368, 25, 15, 1, 0, 0, 0, 0)[:5] == ("short", 15, "refs-as-lanes", 22, 63)
    assert route(65, 1368, 25, 15, 1, 0, 0, 0, 0) == ("short", 15, "read-minor", 2, 684, 2, 0)
    assert route(140000, 10, 110, 15, 1, 0, 0, 0, 0) == ("band", 15, "row-major", 2188, 1, 10, 1)
    assert route(3000, 64, 25, 15, 1, 0, 0, 0, 0) == ("short", 15, "read-minor", 47, 32, 2, 0)
    assert route(20000, 64, 110, 15, 1, 0, 0, 0, 0) == ("band", 15, "row-major", 313, 7, 10, 0)
    assert route(40000, 10, 110, 15, 1, 0, 0, 0, 0) == ("band", 15, "row-major", 625, 4, 3, 0)
    assert route(2000, 10, 25, 15, 1, 0, 0, 0, 0) == ("short", 15, "read-minor", 32, 10, 1, 0)
    assert route(1000000, 10, 110, 0, 1, 0, 0, 0, 1) == ("wide", 0, "row-major", 15625, 1, 10, 1)
    assert rec[(1000000, 10, 110, 0, 1, 0, 0, 0, 1)]["lds_bytes"] == 56320
    assert route(4096, 851, 64, 0, 1, 0, 0, 0, 1) == ("wide", 0, "read-minor", 64, 54, 16, 0)
    # edges: scratch launches, the fused argmin either side of 2 048 and 24 576 waves, row-major from 8 192 reads,
    # refs as lanes below a wave of reads, the wavefront up to 16 384 pairs, the fused entries
    assert [rec[(n, 9, 110, 33, a, 0, 0, 0, 0)]["launches"] for n, a in ((65536, 0), (65537, 1), (131073, 1))] == [1, 2, 3]
    assert [rec[(n, y, 25, 15, 1, 0, 0, 0, 0)]["fused_argmin"] for n in (131008, 131009) for y in (31, 32)] == [0, 0, 1, 0]
    assert [rec[(n, 64, 25, 15, 1, 0, 0, 0, 0)]["fused_argmin"] for n in (1572800, 1572864)] == [0, 1]
    assert [lay(n, 10, 25, 15, 1, 0, 0, 0, 0) for n in (8191, 8192)] == ["read-minor", "row-major"]
    assert [lay(*c, 25, 15, 1, 0, 1, 0, 0) for c in ((63, 64), (64, 65), (63, 63))] == ["refs-as-lanes", "read-minor", "read-minor"]
    assert [fam(*c, 110, 16, 1, 0, 0, 0, 0) for c in ((4096, 4), (3277, 5))] == ["wavefront", "band"]
    assert [(fam(10, y, 25, 15, 1, 1, 0, 0, 0), lay(10, y, 25, 15, 1, 1, 0, 0, 0)) for y in (3, 1368)] == [("short", "read-minor")] * 2
    assert (fam(10, 3, 110, 5, 1, 1, 0, 0, 0), lay(10, 3, 110, 5, 1, 1, 0, 0, 0)) == ("band", "read-minor")
    assert (fam(8192, 3, 25, 15, 1, 1, 0, 0, 0), lay(8192, 3, 25, 15, 1, 1, 0, 0, 0)) == ("short", "row-major")
    assert rec[(10, 3, 110, 33, 1, 1, 0, 0, 0)]["unsupported"] == 1 and rec[(0, 3, 110, 33, 1, 1, 0, 0, 0)]["unsupported"] == 1
    assert fam(10, 3, 110, 0, 1, 1, 0, 0, 1) == "wide" and rec[(10, 3, 300, 0, 1, 1, 0, 0, 1)]["unsupported"] == 1


def test_invariants_of_every_plan_over_the_sweep(exe):
    run = subprocess.run([exe, "sweep"], capture_output=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:], run.stdout[-500:])
    out = dict((ln.rsplit(" ", 1)[0], int(ln.rsplit(" ", 1)[1])) for ln in run.stdout.decode().splitlines())
    # (L, window) pairs x reads x references x {no switch, each switch alone} x entries x argmin
    pairs = sum(L + 2 for L in list(range(1, 41)) + [110, 256, 257])
    assert out["cases"] == pairs * 26 * 17 * 4 * 2 * 2 == 10_813_088
    # every case has exactly one family or is a fused entry's refusal
    assert sum(out["family %d" % f] for f in range(7)) == out["cases"] and out["family 0"] == out["unsupported"] > 100_000
    for f in (_lib.DTW_WAVEFRONT, _lib.DTW_SHORT, _lib.DTW_BAND, _lib.DTW_SCRATCH, _lib.DTW_WIDE):
        assert out["family %d" % f] > 1000, _lib.DTW_FAMILY_NAMES[f]
    assert out["family %d" % _lib.DTW_SHORT_SVM] == 0   # (the fused SVM route has its own launcher)


def test_header_stands_alone_and_every_object_depends_on_it(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    src = tmp_path / "alone.cpp"
    src.write_text('#include "wdx_dtw_plan.h"\nint main() { return wdx::dtw_plan(1, 1, 1, 0, false, wdx::DtwEntry::kMatrix, {}).info.family == 0; }\n')
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "alone")])
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
    hdr = open(os.path.join(CSRC, "wdx_dtw_plan.h")).read()
    assert "hip/" not in hdr and "wdx_common.h\"" not in hdr and "wdx_ctx.h" not in hdr
    assert "wdx_dtw_plan.h" in open(os.path.join(CSRC, "Makefile")).read()
