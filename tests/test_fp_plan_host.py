"""Which kernels a fingerprint call launches, without a GPU: warpdemux_amd/csrc/wdx_fp_plan.h driven by
tests/host/fp_plan_check.cpp -- built with the system C++ compiler under the address and undefined-behaviour sanitizers
(stand-alone: nothing is preloaded).  The program replays the recorded route table profiles/r08a_launch_sequence.txt (every
section rebuilt as a call, its plan expanded through the header's slicing function and compared launch by launch: kernel with
its template arguments, grid, workgroup size), sweeps about 10^6 plans over the accepted parameter domain for what must hold of
every one (its own header lists the sweep and the invariants), and makes every refusal once, code and message.  The library
runs the same plan_fingerprint; what the replay cannot see -- which list each launch takes and feeds -- needs a device."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "fp_plan_check.cpp")
TABLE = os.path.join(ROOT, "profiles", "r08a_launch_sequence.txt")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    out = str(tmp_path_factory.mktemp("fp_plan") / "fp_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", out])
    return out


def test_replay_of_the_route_table_and_sweep_of_the_plan_under_sanitizers(exe):
    run = subprocess.run([exe, TABLE], capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.decode().splitlines()
    # the table's own head line counts 1 642 lines: 162 section heads and 1 480 launches; no launch line is skipped
    table = [ln for ln in open(TABLE).read().splitlines() if ln.strip() and not ln.startswith("#")]
    n_sections = sum(ln.startswith("== ") for ln in table)
    assert (n_sections, len(table)) == (162, 1642)
    assert lines[0] == "162 sections %d launches" % (len(table) - n_sections) == "162 sections 1480 launches", lines[0]
    words = lines[1].split()
    assert words[1] == "points:" and int(words[0]) > 900000 and all(int(words[i]) > 10000 for i in (2, 4, 6)), lines[1]
    assert lines[2] == "13 refusals", lines[2]
    # printed, not asserted: workgroups per CU by the 1 280-byte LDS granule rule (DESIGN.md 8 carries the open question)
    assert any(ln.startswith("granules striding") and "capP 1856 nbt 1  lds  53904 B" in ln for ln in lines[3:]), lines[3:]


def test_the_header_is_host_only():
    hdr = open(os.path.join(CSRC, "wdx_fp_plan.h")).read()
    assert "hip/" not in hdr and "wdx_common.h" not in hdr and "wdx_ctx.h" not in hdr
    common = open(os.path.join(CSRC, "wdx_common.h")).read()
    assert '#include "wdx_fp_plan.h"' in common
    launch = open(os.path.join(CSRC, "wdx_fingerprint_launch.inc")).read()
    for gone in ("stage_big0", "stage_big1", "stage_stream", "stage_retry", "fill_fast_set", "fast_attr_set"):
        assert gone not in launch, gone
