"""What a barycenter step does with its host labels (warpdemux_amd/csrc/wdx_dba_plan.h: dba_plan), without a GPU.

tests/host/dba_plan_check.cpp is built with the system C++ compiler under the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded) and run as a child process.  Over a sweep of (label sizes, L, window) the program itself checks
what must hold of every plan (the invariants are numbered at its head): the word counts, the route, every padded row in exactly one
pass, no pass beyond the stated code-block bound, every piece inside the workspace and the workspace within the stated bound, each
refusal with its code and message.  The header stands alone and is a dependency of every object of the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "dba_plan_check.cpp")


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    return cxx


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dba_plan") / "dba_plan_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", out])
    run = subprocess.run([out], capture_output=True)
    assert run.returncode == 0, (run.returncode, run.stderr.decode()[-3000:], run.stdout.decode()[-500:])
    return dict((ln.rsplit(" ", 1)[0], int(ln.rsplit(" ", 1)[1])) for ln in run.stdout.decode().splitlines())


def test_invariants_of_every_plan(report):
    assert report["failures"] == 0 and report["checks"] > 1_000_000, report


def test_the_sweep_met_what_it_claims(report):
    """a sweep that never built a plan of several passes, of two words, on the general route or at the longest series proves nothing
    of them"""
    assert report["plans"] >= 280, report
    assert report["multi_pass"] >= 3 and report["general"] >= 100 and report["two_words"] >= 50 and report["at_max_l"] >= 20, report
    assert report["empty_labels"] > 10 and report["unlabelled"] > 100 and report["beyond_medoid_cap"] >= 1, report


def test_header_stands_alone_and_every_object_depends_on_it(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "wdx_dba_plan.h"\nint main() { const int32_t l[2] = {0, 0}; '
                   'return wdx::dba_plan(l, 2, 1, 70, 32, true, true, false).words != 2; }\n')
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "alone")])
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
    hdr = open(os.path.join(CSRC, "wdx_dba_plan.h")).read()
    assert "hip/" not in hdr and "wdx_common.h\"" not in hdr and "wdx_ctx.h" not in hdr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "wdx_dba_plan.h" in mk and "wdx_dba.hip" in mk
