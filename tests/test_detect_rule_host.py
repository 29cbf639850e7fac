"""Boundary detection without a GPU: the ABI's names, the parameter domain, and the NumPy restatement of the rule
(tests/helpers/detect_rule.py, written from include/wdx.h) on the synthetic generator and on hand-made rows.  The kernel is held
to the restatement in tests/test_gpu_detect.py."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from helpers import detect_rule as dr
from warpdemux_amd import _lib, sig_proc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wdx_detect_rows", "wdx_detect_rows_adc", "wdx_detect_batch", "wdx_detect_batch_adc")


def _header():
    return open(os.path.join(ROOT, "include", "wdx.h")).read()


def test_names_constants_and_struct():
    hdr, L = _header(), _lib.load()
    declared = set(re.findall(r"\b(wdx_detect[a-z0-9_]*)\s*\(", hdr))
    assert declared == set(NAMES) == {e for e in _lib.EXPORTS if e.startswith("wdx_detect")}
    for name in NAMES:
        assert hasattr(L, name), name
        assert not name.endswith("_dev") and not name.endswith("_device")     # (the closed tables of the *_dev entries)
    assert L.wdx_abi_version() == _lib.ABI_VERSION == 4

    def define(name):
        return int(re.search(r"^#define\s+%s\s+(\d+)" % name, hdr, flags=re.M).group(1))

    assert define("WDX_K_DETECT") == _lib.K_DETECT == 21
    assert define("WDX_DETECT_MAX_TRACE") == _lib.DETECT_MAX_TRACE == 16384
    codes = ("OK", "SHORT", "NO_START", "NO_ROOM", "NO_POLYA")
    assert [define("WDX_DETECT_" + c) for c in codes] == [getattr(_lib, "DETECT_" + c) for c in codes] == [getattr(dr, c) for c in codes]
    assert sorted(sig_proc.DETECT_FAIL_REASONS) == [0, 1, 2, 3, 4] and sig_proc.DETECT_FAIL_REASONS[0] == ""
    body = hdr[hdr.index("typedef struct wdx_detect_params {"): hdr.index("} wdx_detect_params;")]
    fields = re.findall(r"^\s*(int32_t|float)\s+(\w+);", body, flags=re.M)
    assert [f[1] for f in fields] == [f[0] for f in _lib.DetectParamsC._fields_] == [f.name for f in dataclasses.fields(sig_proc.DetectParams)]
    assert [f[0] == "float" for f in fields] == [f[1] is C.c_float for f in _lib.DetectParamsC._fields_]
    assert C.sizeof(_lib.DetectParamsC) == 52
    for words in ("the engine's own rule; parity with ADAPTed unpinned; accuracy on real reads unmeasured",):
        assert words in hdr
        for doc in ("README.md", "INTEGRATION.md"):
            assert words in open(os.path.join(ROOT, doc)).read(), doc


def test_defaults_are_the_prototype_parameters():
    d = dataclasses.asdict(sig_proc.DetectParams())
    assert {k: (int(v) if isinstance(v, bool) else v) for k, v in d.items()} == dr.DEFAULT
    c = sig_proc.DetectParams().to_c()
    assert (c.max_obs_trace, c.quant_per_pa, c.polya_win, c.max_polya_var) == (10000, 8.0, 200, 9.0)


# each bound of the domain: one step inside, one step outside
INSIDE = [dict(max_obs_trace=1), dict(max_obs_trace=16384), dict(quant_per_pa=1e-30), dict(find_start=0), dict(find_start=1),
          dict(step_win=1), dict(step_win=200, polya_win=200), dict(polya_win=1024), dict(min_obs_adapter=8, step_win=8),
          dict(max_obs_adapter=1000, min_obs_adapter=1000), dict(start_win=1), dict(start_win=256), dict(refine=0), dict(refine=4096),
          dict(max_start=0), dict(open_pore_pa=-3.0e38), dict(min_shift_pa=3.0e38), dict(max_polya_var=-1.0)]
OUTSIDE = [dict(max_obs_trace=0), dict(max_obs_trace=16385), dict(quant_per_pa=0.0), dict(quant_per_pa=-1.0), dict(find_start=2),
           dict(find_start=-1), dict(step_win=0), dict(step_win=201, polya_win=200), dict(polya_win=1025),
           dict(min_obs_adapter=7, step_win=8), dict(max_obs_adapter=999, min_obs_adapter=1000), dict(start_win=0), dict(start_win=257),
           dict(refine=-1), dict(refine=4097), dict(max_start=-1), dict(quant_per_pa=float("inf")), dict(open_pore_pa=float("nan")),
           dict(min_shift_pa=float("inf")), dict(max_polya_var=float("-inf")), dict(open_pore_pa=1e39)]


@pytest.mark.parametrize("change", INSIDE, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_domain_inside(change):
    sig_proc.DetectParams(**change).to_c()


@pytest.mark.parametrize("change", OUTSIDE, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_domain_outside(change):
    with pytest.raises(ValueError):
        sig_proc.DetectParams(**change).to_c()


def test_threshold_formulas():
    assert dr.thresholds(dr.DEFAULT) == (1200, 64, 576)
    # the clamps: a threshold beyond what q can reach compares like the clamp value
    assert dr.thresholds(dict(dr.DEFAULT, open_pore_pa=1e30, min_shift_pa=-1e30, max_polya_var=1e30)) == (32768, -65536, 2147483648)
    assert dr.thresholds(dict(dr.DEFAULT, open_pore_pa=-1e30, min_shift_pa=1e30, max_polya_var=-5.0)) == (-32768, 65536, -1)
    assert dr.thresholds(dict(dr.DEFAULT, quant_per_pa=0.3, open_pore_pa=2.5, max_polya_var=7.0))[0] == int(np.rint(np.float32(2.5) * np.float32(0.3)))


def test_rule_sanity_on_the_synthetic_generator():
    """2 000 traces of the synthetic generator, default parameters.  The prototype of the rule measured 98.97 % success, a_start
    exact on all successes and a_end within 12 samples on 96.8 % of them; the bounds leave room for another generator's draws."""
    rows, truth = dr.synth_batch(2024, 2000)
    E = dr.detect_rows(rows, dr.DEFAULT)
    ok = E.ok == 1
    start_exact = (E.a_start[ok] == truth[ok, 0]).mean()
    end_close = (np.abs(E.a_end[ok].astype(np.int64) - truth[ok, 1]) <= 12).mean()
    print("success %.4f, a_start exact %.4f, |a_end - truth| <= 12: %.4f" % (ok.mean(), start_exact, end_close))
    assert ok.mean() >= 0.97
    assert start_exact >= 0.99
    assert end_close >= 0.93
    assert np.array_equal(E.ok == 1, E.code == dr.OK) and np.array_equal(E.a_end >= 0, ok)


def _small(**kw):
    return dict(dr.SMALL, **kw)


def test_a_constant_row_ties_every_g():
    E = dr.detect_one(np.full(64, 100.0, np.float32), _small(min_shift_pa=0.0))
    # s = 0 (100 pA < 150 pA), lo = 8, every g(i) = 800^2 * 64: the smallest index wins, and so does the smallest j of the refinement
    assert E["g_tie"] and E["info"][1] == 8 and E["gain"] == 800.0 ** 2 * 64
    assert (E["code"], E["a_start"], E["a_end"], E["d_tie"]) == (dr.OK, 0, 8, True)
    assert E["info"] == [64, 8, 8 * 800, 8 * 800]
    assert dr.detect_one(np.full(64, 100.0, np.float32), dr.SMALL)["code"] == dr.NO_POLYA      # no shift of 8 pA


def test_infinite_rows_clamp():
    up = dr.detect_one(np.full(64, np.inf, np.float32), dr.SMALL)
    assert up["code"] == dr.NO_START and up["info"] == [64, -1, -1, -1]                      # 32767 >= thr1
    down = dr.detect_one(np.full(64, -np.inf, np.float32), _small(min_shift_pa=0.0))
    assert down["code"] == dr.OK and down["info"] == [64, 8, 8 * -32768, 8 * -32768]
    assert dr.quantise(np.array([np.inf, 4095.9, 4095.875, -4096.0, -np.inf, 0.0625, 0.1875], np.float32), 8.0).tolist() == \
        [32767, 32767, 32767, -32768, -32768, 0, 2]


def test_nan_at_sample_zero_and_the_length_bound():
    row = np.full(64, 100.0, np.float32)
    row[0] = np.nan
    E = dr.detect_one(row, dr.SMALL)
    assert E["code"] == dr.SHORT and E["info"] == [0, -1, -1, -1] and E["a_start"] == -1 and np.isnan(E["gain"])
    assert np.array([E["gain"]]).view(np.uint64)[0] == dr.NAN_BITS
    need = dr.SMALL["start_win"] + dr.SMALL["min_obs_adapter"] + dr.SMALL["polya_win"]
    assert dr.detect_one(np.full(need - 1, 100.0, np.float32), dr.SMALL)["code"] == dr.SHORT
    at = dr.detect_one(np.full(need, 100.0, np.float32), _small(min_shift_pa=0.0))
    assert at["code"] == dr.OK and at["info"][0] == need
    # the cap: a row longer than max_obs_trace is cut there, with or without a NaN behind it
    assert dr.detect_one(np.full(64, 100.0, np.float32), _small(max_obs_trace=need - 1))["code"] == dr.SHORT


def test_small_generator_reaches_every_code_and_both_ties():
    rows, lengths = dr.small_batch(7, 1000)
    E = dr.detect_rows(rows, dr.SMALL)
    assert sorted(set(E.code.tolist())) == [0, 1, 2, 3, 4]
    assert E.g_tie.any() and E.d_tie.any()
    assert set(dr.SMALL_LENGTHS) <= set(lengths.tolist())
    assert np.array_equal(E.info[:, 0], lengths)


def test_no_device_is_an_error_not_a_fallback():
    if _lib.load().wdx_device_count() > 0:
        # (with a device the host form answers; tests/test_gpu_detect.py compares it)
        assert len(sig_proc.detect_batch(np.full((1, 64), 100.0, np.float32), sig_proc.DetectParams(**dr.SMALL))) == 1
        return
    with pytest.raises(_lib.WdxError):
        sig_proc.detect_batch(np.full((1, 64), 100.0, np.float32))
