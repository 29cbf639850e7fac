"""What a leave-one-out nearest-neighbour call does with its sizes (warpdemux_amd/csrc/wdx_loo_plan.h: loo_plan), without a GPU.

tests/host/loo_plan_check.cpp is built with the system C++ compiler under the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded) and run as a child process.  Over a sweep of (n, L, window, option) the program itself checks
what must hold of every plan (the invariants are numbered at its head): every unordered chunk pair in exactly one tile and every
row offered every other row exactly once, the general route's blocks covering each padded row once within the 96 MiB bound, every
workspace piece inside the stated bound, the keys' order, each refusal with its code and message.  The header stands alone and is
a dependency of every object of the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "loo_plan_check.cpp")


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    return cxx


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("loo_plan") / "loo_plan_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", out])
    run = subprocess.run([out], capture_output=True)
    assert run.returncode == 0, (run.returncode, run.stderr.decode()[-3000:], run.stdout.decode()[-500:])
    return dict((ln.rsplit(" ", 1)[0], int(ln.rsplit(" ", 1)[1])) for ln in run.stdout.decode().splitlines())


def test_invariants_of_every_plan(report):
    assert report["failures"] == 0 and report["checks"] > 1_000_000, report


def test_the_sweep_met_what_it_claims(report):
    """a sweep that never built a plan at the cap, on the general route or of several row blocks proves nothing of them"""
    assert report["plans"] >= 100 and report["at_cap"] >= 6 and report["pair_checked"] >= 50, report
    assert report["general"] >= 40 and report["multi_block"] >= 10 and report["blocks"] > report["general"], report


def test_header_stands_alone_and_every_object_depends_on_it(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "wdx_loo_plan.h"\nint main() { const wdx::LooPlan P = wdx::loo_plan(200, 110, 15, true, false, false); '
                   'return !(P.rc == 0 && P.tile_count() == 10 && !P.general); }\n')
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "alone")])
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
    hdr = open(os.path.join(CSRC, "wdx_loo_plan.h")).read()
    assert "hip/" not in hdr and "wdx_common.h\"" not in hdr and "wdx_ctx.h" not in hdr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "wdx_loo_plan.h" in mk and "wdx_dtw_loo.hip" in mk
