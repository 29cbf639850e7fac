"""The slot plan of the optimal change-points (WDX_OPT_REFINE_OPTIMAL_CPTS), without a GPU:
warpdemux_amd/csrc/wdx_refine_optimal_plan.h swept by tests/host/optimal_plan_check.cpp -- built with the system C++ compiler
under the address and undefined-behaviour sanitizers (stand-alone: nothing is preloaded) -- against the restatement in
tests/helpers/optimal_plan.py, field by field, and the figures the comments and tests/test_gpu_optimal_batch.py rely on."""
import itertools
import os
import shutil
import subprocess

import numpy as np

from helpers import optimal_plan as op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "optimal_plan_check.cpp")
READS = (1, 2, 9, 199, 200, 2048, 2049, 10 ** 6)
LENS = (1, 63, 64, 65, 2047, 2048, 2049, 11264, 16383, 16384)
BKPS = (1, 25, 60, 253)
MAX_SLOTS = (0, 1, 2)


def test_plan_over_its_edges_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "optimal_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe])
    run = subprocess.run([exe], capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.array([ln.split() for ln in run.stdout.decode().splitlines()], dtype=np.int64)
    cases = list(itertools.product(READS, LENS, BKPS, MAX_SLOTS))
    assert got.shape == (len(cases), 8) and run.stderr.decode().strip().endswith("%d cases" % len(cases))
    assert [tuple(r) for r in got[:, :4].tolist()] == cases, "every case once, in order"
    for (n_reads, max_len, B, max_slots), (cap, slot_bytes, slots, nbytes) in zip(cases, got[:, 4:].tolist()):
        want = op.optimal_plan(n_reads, max_len, B, max_slots)
        what = (n_reads, max_len, B, max_slots)
        assert cap == want["cap"], what
        assert slot_bytes == want["slot_bytes"], what
        assert slots == want["slots"], what
        assert nbytes == want["bytes"], what
        assert nbytes <= 256 << 20 and slots >= 1, what
    # both storage forms and a plan bounded by each of its four limits occur
    cap, slots = got[:, 4], got[:, 6]
    assert (cap <= 2047).any() and (cap > 2047).any()
    assert (slots == 2048).any() and (slots == got[:, 0]).any() and (slots == got[:, 3]).any()
    assert ((slots < 2048) & (slots < got[:, 0]) & (got[:, 3] == 0)).any(), "bounded by the scratch buffer"


def test_figures_the_comments_and_the_batch_tests_quote():
    MiB = float(1 << 20)
    # the largest slot: B = 253 at 16 384 samples -- 8 815 360 bytes, 8.41 MiB, 30 workgroups
    big = op.optimal_plan(10 ** 6, 16384, 253)
    assert big["cap"] == 16384 and big["slot_bytes"] == 8815360 and 8.0 < big["slot_bytes"] / MiB < 9.0
    assert big["slots"] == 30 == (256 << 20) // 8815360 and big["bytes"] <= 256 << 20
    # the tRNA parameters (B = 25) with one window at the cap: 199 workgroups
    trna = op.optimal_plan(10 ** 6, 16384, 25)
    assert trna["slot_bytes"] == 1343744 and trna["slots"] == 199 == op.optimal_plan(420, 16384, 25)["slots"]
    # ... and every batch of 420 reads whose longest row has 15 745 .. 16 384 samples gives a workgroup a third read
    assert max(op.optimal_plan(420, L, 25)["slots"] for L in range(15745, 16385)) == 207
    assert op.optimal_plan(420, 11265, 25)["slots"] == 288, "a shorter longest row: more, smaller slots"
    # tails in LDS (cap <= 2047, that is max_len <= 1984): the path table alone; one sample more and the value rows follow it
    small = op.optimal_plan(10 ** 6, 1984, 25)
    assert small["cap"] == 1984 and small["slot_bytes"] == 99328 and small["slots"] == 2048
    assert op.optimal_plan(10 ** 6, 1985, 25)["slot_bytes"] == 168192   # 102 464 + 4 x 2049 x 8, to 256 bytes
    assert op.optimal_plan(9, 4000, 25)["slots"] == 9 and op.optimal_plan(0, 4000, 25)["slots"] == 1
