"""The host side of the wide-window DTW kernel (WDX_OPT_WIDE_DTW), without a GPU.

(1) warpdemux_amd/csrc/wdx_dtw_wide.h -- which dispatches take the kernel, its strips, its LDS block and the waves a CU holds
-- swept by tests/host/dtw_wide_check.cpp over every L in 1 .. 300, window in 0 .. 303 and option in {0, 1}; the program is
built with the system C++ compiler under the address and undefined-behaviour sanitizers (stand-alone: nothing is preloaded)
and its answers are compared with the rule as restated here.
(2) the ``wide_dtw=`` keyword of DemuxEngine, MinibatchPipeline, Feeder and LiveDemux is validated before any context is
created: a non-bool raises ValueError on a machine that has no GPU to create a context on.
(3) the header, the ctypes layer and the kernel's constants agree."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from warpdemux_amd import _lib, parallel_distances as pdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "dtw_wide_check.cpp")
LDS_PER_CU = 160 * 1024


def test_wide_plan_over_its_whole_domain_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "dtw_wide_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe])
    run = subprocess.run([exe], capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.array([ln.split() for ln in run.stdout.decode().splitlines()], dtype=np.int64)
    assert got.shape == (300 * 304 * 2, 8) and run.stderr.decode().strip().endswith("%d cases" % got.shape[0])
    L, window, option, eligible, strips, lds, waves, w_eff = got.T
    # every case once
    assert len({(a, b, c) for a, b, c in zip(L.tolist(), window.tolist(), option.tolist())}) == got.shape[0]
    assert L.min() == 1 and L.max() == 300 and window.min() == 0 and window.max() == 303
    # the rule: the reference's window (None / 0 / beyond L = unbanded = L); eligible iff the option is 1, the effective
    # window exceeds 32 and L <= 256
    want_w = np.where((window <= 0) | (window > L), L, window)
    assert np.array_equal(w_eff, want_w)
    want = (option == 1) & (want_w > 32) & (L <= 256)
    assert np.array_equal(eligible != 0, want)
    assert want.sum() > 10_000 and (~want).sum() > 10_000
    e = want
    assert np.array_equal(strips[e], (L[e] + 31) // 32) and (strips[~e] == 0).all()
    assert np.array_equal(lds[e], 512 * L[e]) and (lds[~e] == 0).all()
    assert (lds <= LDS_PER_CU).all()                                      # everywhere
    assert (waves[e] >= 1).all() and (waves[e] * lds[e] <= LDS_PER_CU).all() and (waves[~e] == 0).all()
    assert ((waves[e] + 1) * lds[e] > LDS_PER_CU - 1280 * (waves[e] + 1)).all()     # no wave forgotten (1280-byte granules)
    # the figures the documents quote
    pick = lambda l, w: got[(L == l) & (window == w) & (option == 1)][0]
    assert pick(110, 0)[3:7].tolist() == [1, 4, 56320, 2]
    assert pick(256, 0)[3:7].tolist() == [1, 8, 131072, 1]
    assert pick(40, 33)[3:7].tolist() == [1, 2, 20480, 8]
    assert pick(257, 0)[3] == 0 and pick(110, 32)[3] == 0 and pick(33, 33)[3] == 1 and pick(32, 0)[3] == 0


def test_constants_agree_between_header_ctypes_layer_and_kernel_header():
    hdr = open(os.path.join(ROOT, "include", "wdx.h")).read()
    val = lambda name: int(re.search(r"^#define\s+%s\s+(\d+)" % name, hdr, flags=re.M).group(1))
    assert val("WDX_OPT_WIDE_DTW") == 24 == _lib.OPT_WIDE_DTW
    assert val("WDX_DTW_WIDE") == 6 == _lib.DTW_WIDE and _lib.DTW_FAMILY_NAMES[6] == "wide"
    assert val("WDX_DTW_WIDE_MAX_L") == 256 == _lib.DTW_WIDE_MAX_L
    assert val("WDX_ABI_VERSION") == 4 == _lib.ABI_VERSION
    assert "wdx_dtw_wide.h" in open(os.path.join(CSRC, "Makefile")).read()


class _NoContext:
    """_lib.Context replaced by a class that fails the test when it is instantiated"""

    def __init__(self, *a, **k):
        raise AssertionError("a context was created before the keyword was validated")


@pytest.mark.parametrize("bad", [1, 0, None, "yes", 33, 1.0])
def test_wide_dtw_keyword_is_validated_before_any_context_exists(monkeypatch, bad):
    from warpdemux_amd import engine, feeder, live, pipeline

    monkeypatch.setattr(_lib, "Context", _NoContext)
    refs = np.zeros((3, 40))
    with pytest.raises(ValueError, match="wide_dtw"):
        engine.DemuxEngine(refs, None, 0.1, wide_dtw=bad)
    with pytest.raises(ValueError, match="wide_dtw"):
        pipeline.MinibatchPipeline(refs, None, 0.1, wide_dtw=bad)
    with pytest.raises(ValueError, match="wide_dtw"):
        feeder.Feeder(refs, None, 0.1, wide_dtw=bad)
    with pytest.raises(ValueError, match="wide_dtw"):
        live.LiveDemux(refs, None, 0.1, wide_dtw=bad)
    with pytest.raises(ValueError, match="wide_dtw"):
        pdist.nearest_reference(np.zeros((2, 40)), refs, None, 0.1, wide_dtw=bad if bad is not None else "no")
