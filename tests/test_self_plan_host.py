"""What a self-distance-matrix call does with its sizes (warpdemux_amd/csrc/wdx_self_plan.h: self_plan), without a GPU.

tests/host/self_plan_check.cpp is built with the system C++ compiler under the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded) and run as a child process.  Over n in {0, 1, 63, 64, 65, 4 097, 65 536}, sizes around the
general route's block edges, both routes and three lengths the program itself checks what must hold of every plan (the invariants
are numbered at its head): every unordered pair of rows in exactly one decoded tile and every entry of the matrix written exactly
once (n <= 4 097), the workspace within its pieces and its stated bound, the general route's row blocks, each refusal with its code
and message (65 537 rows among them).  The header stands alone and is a dependency of every object of the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "self_plan_check.cpp")


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    return cxx


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("self_plan") / "self_plan_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", out])
    run = subprocess.run([out], capture_output=True)
    assert run.returncode == 0, (run.returncode, run.stderr.decode()[-3000:], run.stdout.decode()[-500:])
    return dict((ln.rsplit(" ", 1)[0], int(ln.rsplit(" ", 1)[1])) for ln in run.stdout.decode().splitlines())


def test_invariants_of_every_plan(report):
    assert report["failures"] == 0 and report["checks"] > 100_000, report


def test_the_sweep_met_what_it_claims(report):
    """a sweep that never built a plan at the cap, never checked row pairs or never cut row blocks proves nothing of them"""
    assert report["plans"] >= 50, report
    assert report["at_cap"] >= 4 and report["pair_checked"] >= 20, report
    assert report["blocks"] >= 40, report
    assert report["tiles"] >= 4 * (1024 * 1025 // 2), report


def test_header_stands_alone_and_every_object_depends_on_it(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "wdx_self_plan.h"\nint main() { return wdx::self_plan(65, 5, 65, 0, true, false, false).tile_count() != 3; }\n')
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "alone")])
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
    hdr = open(os.path.join(CSRC, "wdx_self_plan.h")).read()
    assert "hip/" not in hdr and "wdx_common.h\"" not in hdr and "wdx_ctx.h" not in hdr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "wdx_self_plan.h" in mk and "wdx_dtw_self.hip" in mk and "wdx_dtw_tile.h" in mk
