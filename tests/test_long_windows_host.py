"""``long_windows`` on the host side: the constants against include/wdx.h, `SegParams.from_spc`'s two thresholds, and the
keyword on the four classes -- accepted before a context, a ring or a process exists (no GPU)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from warpdemux_amd import _lib, engine, feeder, live, pipeline, sig_proc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wdx.h")


def _define(name):
    with open(HEADER) as fh:
        m = re.search(rf"^#define {name} (\d+)\b", fh.read(), re.M)
    assert m, name
    return int(m.group(1))


def test_constants_match_the_header():
    assert _lib.OPT_LONG_WINDOWS == 20 == _define("WDX_OPT_LONG_WINDOWS")
    assert sig_proc.MAX_LONG_ADAPTER_SAMPLES == 65536 == _define("WDX_MAX_LONG_ADAPTER_SAMPLES")
    assert sig_proc.MAX_ADAPTER_SAMPLES == 16384 == _define("WDX_MAX_ADAPTER_SAMPLES")
    assert _define("WDX_ABI_VERSION") == 4


def _spc(max_obs_trace, padding=100):
    return SimpleNamespace(
        sig_extract=SimpleNamespace(padding=padding, normalization="none"),
        core=SimpleNamespace(sig_norm_outlier_thresh=5.0, max_obs_trace=max_obs_trace),
        segmentation=SimpleNamespace(num_events=110, min_obs_per_base=15, running_stat_width=30, accept_less_cpts=False,
                                     consensus_refinement=False, normalization="mean", barcode_num_events=25))


def test_from_spc_thresholds():
    with pytest.raises(NotImplementedError, match="16384") as e:
        sig_proc.SegParams.from_spc(_spc(40000))
    assert "WDX_MAX_ADAPTER_SAMPLES" in str(e.value) and "40200 samples" in str(e.value)
    with pytest.raises(NotImplementedError, match="16384"):
        sig_proc.SegParams.from_spc(_spc(40000), long_windows=False)
    p = sig_proc.SegParams.from_spc(_spc(40000), long_windows=True)
    assert (p.padding, p.num_events, p.min_obs_per_base, p.running_stat_width) == (100, 110, 15, 30)
    assert sig_proc.SegParams.from_spc(_spc(65336), long_windows=True).padding == 100     # 65 336 + 200 = 65 536: the cap itself
    with pytest.raises(NotImplementedError, match="65536") as e:
        sig_proc.SegParams.from_spc(_spc(70000), long_windows=True)
    assert "WDX_MAX_LONG_ADAPTER_SAMPLES" in str(e.value)
    with pytest.raises(NotImplementedError, match="65536"):
        sig_proc.SegParams.from_spc(_spc(65337), long_windows=True)
    assert sig_proc.SegParams.from_spc(_spc(15000)) == sig_proc.SegParams.from_spc(_spc(15000), long_windows=True)


class _RuleDone(Exception):
    """raised in place of the library: the constructor got past its own checks"""


@pytest.mark.parametrize("long_windows", [False, True])
def test_the_four_constructors_take_the_keyword(monkeypatch, long_windows):
    def stop(*a, **k):
        raise _RuleDone()

    monkeypatch.setattr(_lib, "load", stop)
    monkeypatch.setattr(_lib, "Context", stop)
    fake_torch = SimpleNamespace(cuda=SimpleNamespace(is_available=lambda: True), device=lambda *a: None)
    monkeypatch.setattr(engine, "_torch", lambda: fake_torch)
    refs = np.zeros((3, 25))
    for cls in (pipeline.MinibatchPipeline, feeder.Feeder, live.LiveDemux, engine.DemuxEngine):
        obj = cls.__new__(cls)
        with pytest.raises(_RuleDone):
            obj.__init__(refs=refs, long_windows=long_windows)
    with pytest.raises(TypeError):
        pipeline.MinibatchPipeline.__new__(pipeline.MinibatchPipeline).__init__(refs=refs, long_window=True)


def test_module_level_calls_take_the_keyword():
    import inspect

    for fn in (sig_proc.fingerprint_batch, sig_proc.fingerprint_batch_adc, sig_proc.demux_batch, sig_proc.demux_batch_adc,
               sig_proc.detect_results_to_fpt_batch):
        assert inspect.signature(fn).parameters["long_windows"].default is False, fn.__name__


def test_the_option_is_put_back_after_a_call_even_when_it_raises():
    """`Context.long_windows_for_call` on a stand-in context: set for the call, restored behind it, untouched when equal"""
    calls = []
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.long_windows = False
    ctx.set_option = lambda opt, val=1: (calls.append((opt, val)), setattr(ctx, "long_windows", bool(val)))
    with ctx.long_windows_for_call(True):
        assert ctx.long_windows
    with pytest.raises(KeyError):
        with ctx.long_windows_for_call(True):
            raise KeyError("x")
    assert not ctx.long_windows
    with ctx.long_windows_for_call(False):
        pass
    assert calls == [(20, 1), (20, 0), (20, 1), (20, 0)]
    ctx._h = None   # (nothing to destroy)
