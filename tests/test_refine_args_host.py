"""The refinement-parameter checks of every entry point (warpdemux_amd/csrc/wdx_refine_args.h: refine_seg_params) without a
GPU: tests/host/refine_args_check.cpp is built with the system C++ compiler under the address and undefined-behaviour
sanitizers and run over null / zero / negative / limit values of every field; its answers are compared with the rule as
stated here.  The program itself asserts that a refused call leaves *pv alone and that an accepted one copies every other
field.  (tail_ready reads the context, which holds HIP handles, and is covered on the device: test_gpu_entry_preconditions.py.)"""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "refine_args_check.cpp")
I32 = np.iinfo(np.int32)
QUERY, KEEP = 1, 2      # kRefineQuery, kRefineKeep
INVALID = -1            # WDX_ERR_INVALID


def _cases():
    """columns: p_null rp_given query_null n_query barcode_keep_events checks barcode_num_events"""
    edge = [I32.min, -1, 0, 1, 2, 96, 97, 254, 255, I32.max]
    axes = ([0, 1], [0, 1], [0, 1], edge, edge, [0, QUERY, KEEP, QUERY | KEEP], [I32.min, 0, 1, 25, I32.max])
    return np.stack([g.ravel() for g in np.meshgrid(*[np.asarray(a, np.int64) for a in axes], indexing="ij")], axis=1)


def _rule(c):
    """code, K of *pv (-777: refused), message: 1 a null p or a null query, 2 n_query < 1, 3 barcode_keep_events < 1 -- in that
    order, the last two only where the site asks for them, and none of the three without refinement parameters but the null p"""
    p_null, rp, q_null, n_query, keep, checks, K = c.T
    which = np.zeros(len(c), np.int64)
    which = np.where((which == 0) & ((p_null == 1) | ((rp == 1) & (q_null == 1))), 1, which)
    which = np.where((which == 0) & (rp == 1) & ((checks & QUERY) != 0) & (n_query < 1), 2, which)
    which = np.where((which == 0) & (rp == 1) & ((checks & KEEP) != 0) & (keep < 1), 3, which)
    ok = which == 0
    return np.stack([np.where(ok, 0, INVALID), np.where(ok, np.where(rp == 1, keep, K), -777), which], axis=1)


def test_refine_seg_params_over_its_domain_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "refine_args_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe])
    cases = _cases()
    run = subprocess.run([exe], input=np.ascontiguousarray(cases, dtype="<i8").tobytes(), capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr.decode().strip().endswith("%d cases" % cases.shape[0]), run.stderr[-2000:]
    got = np.frombuffer(run.stdout, dtype="<i8").reshape(-1, 3)
    want = _rule(cases)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (cases[bad[0]], got[bad[0]], want[bad[0]])
    # every answer occurs, and a site that asks for neither range check is refused a null pointer only
    assert set(got[:, 2].tolist()) == {0, 1, 2, 3}
    lax = cases[:, 5] == 0
    assert set(got[lax, 2].tolist()) == {0, 1}
