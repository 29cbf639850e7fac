"""What a device MLP fit does with its sizes (warpdemux_amd/csrc/wdx_mlp_fit_plan.h: mlp_fit_plan), without a GPU.

tests/host/mlp_fit_plan_check.cpp is built with the system C++ compiler under the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded) and run as a child process.  Over 12 layer shapes x 10 batch sizes x 13 row counts (and one fit
of a hundred million rows) the program itself checks what must hold of every plan (the invariants are numbered at its head): the
steps cover the rows once, every workspace piece is disjoint and inside the stated bound, the grids cover every batch row and
every tile of every weight matrix once, every slot is its own, the LDS within 160 KiB, and each refusal with its code and
message.  The header stands alone and is a dependency of every object of the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "mlp_fit_plan_check.cpp")


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    return cxx


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mlp_fit_plan") / "mlp_fit_plan_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", out])
    run = subprocess.run([out], capture_output=True)
    assert run.returncode == 0, (run.returncode, run.stderr.decode()[-3000:], run.stdout.decode()[-500:])
    return dict((ln.rsplit(" ", 1)[0], int(ln.rsplit(" ", 1)[1])) for ln in run.stdout.decode().splitlines())


def test_invariants_of_every_plan(report):
    assert report["failures"] == 0 and report["checks"] > 50_000, report


def test_the_sweep_met_what_it_claims(report):
    """a sweep that never planned a short last batch, a clipped batch, whole tiles, two hidden layers, one output unit or the
    largest batch, or never refused, proves nothing of them"""
    assert report["plans"] == 12 * 10 * 13 + 1, report
    assert report["short_last"] >= 300 and report["batch_clipped"] >= 300 and report["whole_tiles"] >= 10, report
    assert report["two_hidden"] >= 300 and report["one_unit"] >= 300 and report["at_max_batch"] >= 100, report
    assert report["refusals"] >= 28, report


def test_header_stands_alone_and_every_object_depends_on_it(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "wdx_mlp_fit_plan.h"\nint main() { return wdx::mlp_fit_plan(4, 4, nullptr, false, false, false, false).rc != WDX_ERR_INVALID; }\n')
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "alone")])
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
    hdr = open(os.path.join(CSRC, "wdx_mlp_fit_plan.h")).read()
    assert "hip/" not in hdr and "wdx_common.h\"" not in hdr and "wdx_ctx.h" not in hdr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "wdx_mlp_fit_plan.h" in mk and "wdx_mlp_fit.hip" in mk
