"""``long_windows`` for the consensus-refinement branch on the host side (no GPU): the constant against include/wdx.h, the
keyword on `fingerprint_refine_batch`, the per-call context manager, the four owning objects setting both options -- and
the rule that says which option raises the cap of a call (warpdemux_amd/csrc/wdx_window.h: a refining call looks at
WDX_OPT_LONG_REFINE_WINDOWS only, a plain call at WDX_OPT_LONG_WINDOWS only), checked by a stand-alone program built with the
system compiler under the address and undefined-behaviour sanitizers (tests/host/long_cap_check.cpp)."""
import inspect
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from warpdemux_amd import _lib, engine, feeder, live, pipeline, sig_proc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wdx.h")
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")


def _define(name):
    with open(HEADER) as fh:
        m = re.search(rf"^#define {name} (\d+)\b", fh.read(), re.M)
    assert m, name
    return int(m.group(1))


def test_the_constant_matches_the_header():
    assert _lib.OPT_LONG_REFINE_WINDOWS == 21 == _define("WDX_OPT_LONG_REFINE_WINDOWS")
    assert _lib.OPT_LONG_WINDOWS == 20 == _define("WDX_OPT_LONG_WINDOWS")      # unchanged
    assert _define("WDX_ABI_VERSION") == 4


def test_refine_calls_take_the_keyword():
    assert inspect.signature(sig_proc.fingerprint_refine_batch).parameters["long_windows"].default is False
    assert inspect.signature(sig_proc.detect_results_to_fpt_batch).parameters["long_windows"].default is False


def test_detect_results_to_fpt_batch_passes_the_keyword_on_in_its_refine_branch(monkeypatch):
    seen = {}

    class _Done(Exception):
        pass

    def stop(*a, **k):
        seen.update(k)
        raise _Done()

    monkeypatch.setattr(sig_proc, "fingerprint_refine_batch", stop)
    spc = SimpleNamespace(
        sig_extract=SimpleNamespace(padding=100, normalization="none"),
        core=SimpleNamespace(sig_norm_outlier_thresh=5.0, max_obs_trace=40000),
        segmentation=SimpleNamespace(
            num_events=120, min_obs_per_base=9, running_stat_width=18, accept_less_cpts=False, consensus_refinement=True,
            normalization="mean", barcode_num_events=[25, 25], consensus_subseq_match_normalization="mean",
            consensus_subseq_match_penalty=1.5, consensus_subseq_match_psi=[5, 0, 40, 0], consensus_subseq_match_ub_start=18,
            consensus_subseq_match_lb_end=69, consensus_subseq_match_ub_end=97, refinement_optimal_cpts=False))
    dr = [SimpleNamespace(success=True, adapter_start=100, adapter_end=39000)]
    with pytest.raises(_Done):
        sig_proc.detect_results_to_fpt_batch(np.zeros((1, 40200), np.float32), spc, dr, consensus_query=np.arange(84.0),
                                             long_windows=True)
    assert seen["long_windows"] is True
    with pytest.raises(NotImplementedError, match="16384"):       # the default keeps refusing such a configuration
        sig_proc.detect_results_to_fpt_batch(np.zeros((1, 40200), np.float32), spc, dr, consensus_query=np.arange(84.0))


def test_the_refine_option_is_put_back_after_a_call_even_when_it_raises():
    """`Context.long_refine_windows_for_call` on a stand-in context; `long_windows_for_call` keeps touching option 20 only"""
    calls = []
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.long_windows = ctx.long_refine_windows = False

    def set_option(opt, val=1):
        calls.append((opt, val))
        setattr(ctx, {20: "long_windows", 21: "long_refine_windows"}[opt], bool(val))

    ctx.set_option = set_option
    with ctx.long_refine_windows_for_call(True):
        assert ctx.long_refine_windows and not ctx.long_windows
    with pytest.raises(KeyError):
        with ctx.long_refine_windows_for_call(True):
            raise KeyError("x")
    assert not ctx.long_refine_windows
    with ctx.long_refine_windows_for_call(False):
        pass
    with ctx.long_windows_for_call(True):
        assert ctx.long_windows and not ctx.long_refine_windows
    assert calls == [(21, 1), (21, 0), (21, 1), (21, 0), (20, 1), (20, 0)]
    ctx._h = None   # (nothing to destroy)


def test_set_option_tracks_both_options_and_set_long_windows_sets_both(monkeypatch):
    sent = []
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._L = SimpleNamespace(wdx_ctx_set_option=lambda h, o, v: sent.append((o, v)) or 0)
    ctx._h, ctx.pid = 1, os.getpid()
    ctx.long_windows = ctx.long_refine_windows = False
    monkeypatch.setattr(_lib.Context, "handle", property(lambda self: 1))
    ctx.set_long_windows()
    assert sent == [(20, 1), (21, 1)] and ctx.long_windows and ctx.long_refine_windows
    ctx.set_option(_lib.OPT_LONG_REFINE_WINDOWS, 0)
    assert ctx.long_windows and not ctx.long_refine_windows
    ctx._h = None


@pytest.mark.parametrize("cls", [pipeline.MinibatchPipeline, feeder.Feeder, live.LiveDemux, engine.DemuxEngine])
def test_the_owning_objects_set_both_options(cls):
    """wherever an object that owns a context sets option 20 it sets option 21 (one call: Context.set_long_windows)"""
    src = inspect.getsource(inspect.getmodule(cls))
    assert "set_long_windows()" in src and "OPT_LONG_WINDOWS, 1" not in src


def test_cap_rule_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "long_cap_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "host", "long_cap_check.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = {tuple(int(v) for v in line.split()[:3]): tuple(int(v) for v in line.split()[3:]) for line in run.stdout.splitlines()}
    assert len(got) == 8
    short, long = _define("WDX_MAX_ADAPTER_SAMPLES"), _define("WDX_MAX_LONG_ADAPTER_SAMPLES")
    for (refine, lw, lrw), (on, cap, cut) in got.items():
        want_on = lrw if refine else lw                # a refining call: option 21 only; a plain call: option 20 only
        assert on == want_on, (refine, lw, lrw)
        assert cap == (long if want_on else short), (refine, lw, lrw)
        assert cut == cap + 1, (refine, lw, lrw)       # the live tick's int16 staging: the cap of the tick's branch, plus one
    assert got[(1, 1, 0)] == (0, short, short + 1) and got[(0, 0, 1)] == (0, short, short + 1)
    assert got[(1, 0, 1)] == (1, long, long + 1) and got[(0, 1, 0)] == (1, long, long + 1)
