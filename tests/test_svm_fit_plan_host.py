"""What a batched SMO solve does with its problems (warpdemux_amd/csrc/wdx_svm_fit_plan.h: svm_fit_plan), without a GPU.

tests/host/svm_fit_plan_check.cpp is built with the system C++ compiler under the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded) and run as a child process.  Over single problems around every threshold (256 / 257,
2 048 / 2 049, 16 384 rows), a fit-shaped batch, 3 000 small problems and one large problem among small ones the program itself
checks what must hold of every plan (the invariants are numbered at its head): the grid order, the instantiation, the LDS within
160 KiB, the table within its bound, and each refusal with its code and message (16 385 rows among them).  The header stands
alone and is a dependency of every object of the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "svm_fit_plan_check.cpp")


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    return cxx


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("svm_fit_plan") / "svm_fit_plan_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", out])
    run = subprocess.run([out], capture_output=True)
    assert run.returncode == 0, (run.returncode, run.stderr.decode()[-3000:], run.stdout.decode()[-500:])
    return dict((ln.rsplit(" ", 1)[0], int(ln.rsplit(" ", 1)[1])) for ln in run.stdout.decode().splitlines())


def test_invariants_of_every_plan(report):
    assert report["failures"] == 0 and report["checks"] > 10_000, report


def test_the_sweep_met_what_it_claims(report):
    """a sweep that never planned a problem at the cap, never chose one of the instantiations or never refused proves nothing of them"""
    assert report["plans"] >= 37 and report["problems"] >= 3000, report
    assert report["at_cap"] >= 3 and min(report["kernel0"], report["kernel1"], report["kernel2"]) >= 5, report
    assert report["refusals"] >= 29, report


def test_constants_agree_across_the_layers():
    """the cap in the public header, the plan's instantiations and the ctypes layer"""
    import re

    from warpdemux_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "wdx.h")).read()
    assert int(re.search(r"#define\s+WDX_SVM_FIT_MAX_ROWS\s+(\d+)", hdr).group(1)) == _lib.SVM_FIT_MAX_ROWS == 16384
    plan = open(os.path.join(CSRC, "wdx_svm_fit_plan.h")).read()
    kernels = re.search(r"kSvmFitKernels\[kSvmFitKernelCount\] = \{(.*?)\};", plan).group(1)
    assert tuple(tuple(int(v) for v in pair) for pair in re.findall(r"\{(\d+), (\d+)\}", kernels)) == _lib.SVM_FIT_KERNELS
    assert _lib.K_SVM_FIT == 15 and "wdx_svm_solve_device" in _lib.EXPORTS and "wdx_svm_solve" in _lib.EXPORTS


def test_header_stands_alone_and_every_object_depends_on_it(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "wdx_svm_fit_plan.h"\nint main() { return wdx::svm_fit_plan(4, 4, nullptr, 0, nullptr, 0, nullptr, 0, 1e-3, 1, false, false, false).rc; }\n')
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "alone")])
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
    hdr = open(os.path.join(CSRC, "wdx_svm_fit_plan.h")).read()
    assert "hip/" not in hdr and "wdx_common.h\"" not in hdr and "wdx_ctx.h" not in hdr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "wdx_svm_fit_plan.h" in mk and "wdx_svm_fit.hip" in mk
