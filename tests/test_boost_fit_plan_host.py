"""What a device Fpt_Boost fit does with its sizes (warpdemux_amd/csrc/wdx_boost_fit_plan.h: boost_fit_plan), without a GPU.

tests/host/boost_fit_plan_check.cpp is built with the system C++ compiler under the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded) and run as a child process.  Over 6 feature counts x 5 class counts x 5 depths x 8 border counts x
13 row counts the program itself checks what must hold of every admitted plan (the invariants are numbered at its head): the row
chunks cover the rows once and an int32 LDS partial cannot overflow, every workspace piece is disjoint and inside the stated bound
and the cap, the slabs of every level cover every histogram column once within the LDS the launch asks for, the workspace is
monotone in n, and each refusal fires with its code and message.  The header stands alone and is a dependency of every object of
the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "boost_fit_plan_check.cpp")


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    return cxx


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("boost_fit_plan") / "boost_fit_plan_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", out])
    run = subprocess.run([out], capture_output=True)
    assert run.returncode == 0, (run.returncode, run.stderr.decode()[-3000:], run.stdout.decode()[-500:])
    return dict((ln.rsplit(" ", 1)[0], int(ln.rsplit(" ", 1)[1])) for ln in run.stdout.decode().splitlines())


def test_invariants_of_every_plan(report):
    """among them: the 32-bit partial bound for every admitted shape, and a workspace monotone in n"""
    assert report["failures"] == 0 and report["checks"] > 500_000, report


def test_the_sweep_met_what_it_claims(report):
    """a sweep that never planned more than one slab, a short last chunk, whole chunks or a feature without borders, never met
    the workspace cap, or never refused, proves nothing of them"""
    assert report["plans"] + report["cap_refused"] == 6 * 5 * 5 * 8 * 13 + 2, report
    assert report["multi_slab"] >= 1000 and report["short_chunk"] >= 1000 and report["whole_chunks"] >= 1000, report
    assert report["inactive"] >= 1000 and report["cap_refused"] >= 1, report
    assert report["refusals"] == 31, report


def test_the_rows_of_a_pass_are_what_python_names(report):
    from warpdemux_amd import _lib

    assert report["rows"] == _lib.BOOST_FIT_ROWS and report["rows"] << _lib.BOOST_FIT_GRAD_BITS < 1 << 31


def test_header_stands_alone_and_every_object_depends_on_it(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "wdx_boost_fit_plan.h"\nint main() { return wdx::boost_fit_plan(4, 4, nullptr, nullptr, false, false, false, false, false).rc != WDX_ERR_INVALID; }\n')
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "alone")])
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
    hdr = open(os.path.join(CSRC, "wdx_boost_fit_plan.h")).read()
    assert "hip/" not in hdr and "wdx_common.h\"" not in hdr and "wdx_ctx.h" not in hdr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "wdx_boost_fit_plan.h" in mk and "wdx_boost_fit.hip" in mk
