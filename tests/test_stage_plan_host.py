"""What the host-fed paths stage and hand back, without a GPU: warpdemux_amd/csrc/wdx_stage_plan.h swept by
tests/host/stage_plan_check.cpp -- built with the system C++ compiler under the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded, nothing is loaded into Python).  The program itself asserts, point by point: the output
plan over its domain (no two pieces overlap, every offset a multiple of 8, the travelling pieces are exactly the front, and
total / copy_bytes / every offset of the live tick's block equal to the arithmetic the tick did by hand before the plan
existed, transcribed there as plain formulas; the same invariants for a pipeline slot's masks); the delivery (wanted arrays
hold their piece, every other array is untouched, call is -1 without references); and the staging images of seeded batches,
each filled into a block of exactly the stated size (column and row alignment, totals, the staged samples, the columns against
adapter_window, the int16 tick's image against a minibatch's of the same rows)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "stage_plan_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    out = str(tmp_path_factory.mktemp("stage_plan") / "stage_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", out])
    return out


def test_plan_delivery_and_images_under_sanitizers(exe):
    run = subprocess.run([exe], capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    words = run.stderr.decode().split()
    assert words[-1] == "points" and int(words[-2]) > 51_000_000, run.stderr[-200:]
