"""The int16 ADC way in on the GPU: the decode kernels against the NumPy statement of the contract
(`sig_proc.calibrate_adc`), and every ADC route against its float32 counterpart on the calibrated rows -- bit for bit,
over every output, NaN-aware (`_same`) -- plus the CPU oracle on those rows.  Inputs: tests/helpers/adc_inputs.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import adc_inputs
from oracle import wdx_oracle as orc
from warpdemux_amd import _lib, pipeline, sig_proc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 25


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _batches():
    return [("main", adc_inputs.main_batch()), ("long", adc_inputs.long_batch())]


def _rows(b):
    return sig_proc.calibrate_adc(b["adc"], b["row_len"], b["offset"], b["scale"])


def _params(b):
    return sig_proc.SegParams(barcode_num_events=K, padding=b["padding"])


def test_calibrate_adc_dev_equals_the_numpy_statement():
    """decode_adc_kernel through wdx_calibrate_adc_dev: rows on 16-byte boundaries (the 16-byte loads and stores), a stride
    that puts every other row off them (the element loop), packed rows, lengths 0 and stride, the int16 extremes."""
    import torch

    L = _lib.load()
    ctx = _lib.Context(0)
    rng = np.random.default_rng(3)
    for stride in (4096, 4099, 8, 7, 1):
        n = 37
        adc = rng.integers(-32768, 32768, size=(n, stride)).astype(np.int16)
        adc[0, 0], adc[1, 0] = -32768, 32767
        row_len = rng.integers(0, stride + 1, size=n).astype(np.int32)
        row_len[:4] = [stride, 0, min(stride, 9), max(stride - 1, 0)]
        offset = (-240 + rng.uniform(-20, 20, n)).astype(np.float32)
        scale = (0.1755 * (1 + 0.02 * rng.uniform(-1, 1, n))).astype(np.float32)
        want = sig_proc.calibrate_adc(adc, row_len, offset, scale)
        d = [torch.from_numpy(a).cuda() for a in (adc, row_len, offset, scale)]
        out = torch.full((n, stride), 7.0, dtype=torch.float32, device="cuda")
        _lib.check(L.wdx_calibrate_adc_dev(ctx.handle, d[0].data_ptr(), None, d[1].data_ptr(), stride, n, d[2].data_ptr(),
                                           d[3].data_ptr(), out.data_ptr(), None))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), stride
        assert _same(got, want), stride
        # the same reads as packed rows (offsets in multiples of 8, row r holds its row_len[r] samples)
        lens8 = (row_len.astype(np.int64) + 7) // 8 * 8
        off = np.concatenate([[0], np.cumsum(lens8)]).astype(np.int64)
        flat = np.full(int(off[-1]) + 8, 999, dtype=np.int16)
        for r in range(n):
            flat[off[r]:off[r] + row_len[r]] = adc[r, :row_len[r]]
        dflat, doff = torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()
        out.fill_(7.0)
        _lib.check(L.wdx_calibrate_adc_dev(ctx.handle, dflat.data_ptr(), doff.data_ptr(), d[1].data_ptr(), stride, n,
                                           d[2].data_ptr(), d[3].data_ptr(), out.data_ptr(), None))
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy(), want), stride
    ctx.close()


def test_blocking_adc_calls_equal_the_float32_calls():
    refs = np.random.default_rng(8).normal(size=(10, K))
    sig_proc.set_references(refs, 15, 0.1)
    for name, b in _batches():
        p, rows = _params(b), _rows(b)
        want = sig_proc.fingerprint_batch(rows, b["a_s"], b["a_e"], p, success=b["ok"])
        got = sig_proc.fingerprint_batch_adc(b["adc"], b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"], p, success=b["ok"])
        assert _same(got.status, want.status), name
        assert _same(got.fpt, want.fpt) and _same(got.dwell, want.dwell) and _same(got.stats, want.stats), name
        wd = sig_proc.demux_batch(rows, b["a_s"], b["a_e"], p, success=b["ok"], want_dist=True, want_fpt=True)
        for adc in (b["adc"], _pinned(b["adc"])):       # the 2-D copy + decode_adc_kernel, pack_windows_adc_kernel over the bus
            gd = sig_proc.demux_batch_adc(adc, b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"], p, success=b["ok"],
                                          want_dist=True, want_fpt=True)
            assert _same(gd.status, wd.status) and _same(gd.call, wd.call), name
            assert _same(gd.dist, wd.dist) and _same(gd.fpt, wd.fpt), name
        assert _same(wd.fpt, want.fpt) and (want.status == 0).sum() * 2 >= len(want.status), name
    assert want.status[4] == 5 and (want.status[[0, 1, 2, 3]] == 0).all()      # the long batch: 16 385 samples / the capacity edges


def test_a_stride_that_is_no_multiple_of_8_takes_the_element_loop_on_every_way_in():
    """rows of 9 001 samples: every row but each eighth starts off the 16-byte boundaries, so the page-locked minibatch is
    read over the bus by pack_windows_adc_kernel's element loop and the pageable one is decoded by decode_adc_kernel's"""
    b = dict(adc_inputs.main_batch())
    b["adc"] = np.ascontiguousarray(np.pad(b["adc"], ((0, 0), (0, 1)), constant_values=-7))
    assert b["adc"].shape[1] % 8 == 1 and adc_inputs.windows_to_box_ratio(b) < 0.8
    refs = np.random.default_rng(8).normal(size=(10, K))
    sig_proc.set_references(refs, 15, 0.1)
    p, rows = _params(b), _rows(b)
    wd = sig_proc.demux_batch(rows, b["a_s"], b["a_e"], p, success=b["ok"], want_dist=True, want_fpt=True)
    assert (wd.status == 0).sum() * 2 >= len(wd.status)
    for adc in (_pinned(b["adc"]), b["adc"]):
        gd = sig_proc.demux_batch_adc(adc, b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"], p, success=b["ok"],
                                      want_dist=True, want_fpt=True)
        assert _same(gd.status, wd.status) and _same(gd.call, wd.call) and _same(gd.dist, wd.dist) and _same(gd.fpt, wd.fpt)


def _pinned(a):
    buf = pipeline.pinned_empty(a.shape, a.dtype)
    np.copyto(buf, a)
    return buf


def test_pipelined_adc_minibatches_equal_the_float32_pipeline_three_ways_in():
    """MinibatchPipeline.submit_adc with a pageable minibatch (2-D copy, decode_adc_kernel), a page-locked one
    (pack_windows_adc_kernel over the bus) and rows the caller packed (flat copy, decode_adc_kernel), and `run` on a mix of
    float32 and int16 minibatches."""
    refs = np.random.default_rng(8).normal(size=(10, K))
    for name, b in _batches():
        p, rows = _params(b), _rows(b)
        pipe = pipeline.MinibatchPipeline(refs, 15, 0.1, p)
        pipe.submit(0, rows, b["a_s"], b["a_e"], success=b["ok"], want_fpt=True)
        want = pipe.wait(0)
        cal = (b["row_len"], b["offset"], b["scale"])
        pipe.submit_adc(0, b["adc"], *cal, b["a_s"], b["a_e"], success=b["ok"], want_fpt=True)
        pipe.submit_adc(1, _pinned(b["adc"]), *cal, b["a_s"], b["a_e"], success=b["ok"], want_fpt=True)
        got = [pipe.wait(0), pipe.wait(1)]
        flat, row_off, r_len, r_win, a_s2, a_e2 = adc_inputs.pack_rows(b)
        pipe.submit_adc(0, flat, r_len, b["offset"], b["scale"], a_s2, a_e2, success=b["ok"], want_fpt=True, row_off=row_off,
                        row_win=r_win)
        got.append(pipe.wait(0))
        got += list(pipe.run([(b["adc"], *cal, b["a_s"], b["a_e"], b["ok"], True, True),
                              (rows, b["a_s"], b["a_e"], b["ok"], True, True),
                              (_pinned(b["adc"]), *cal, b["a_s"], b["a_e"], b["ok"], True, True)]))
        assert len(got) == 6
        for way, g in enumerate(got):
            assert _same(g.status, want.status) and _same(g.call, want.call), (name, way)
            assert _same(g.dist, want.dist) and _same(g.fpt, want.fpt), (name, way)
        assert (want.status == 0).sum() * 2 >= len(want.status), name
        with pytest.raises(ValueError, match="multiples of 8"):
            pipe.submit_adc(0, np.concatenate([flat, flat[:8]]), r_len, b["offset"], b["scale"], a_s2, a_e2, row_off=row_off + 4)
        pipe.close()


def test_adc_fingerprints_equal_the_cpu_oracle_on_the_calibrated_rows():
    """the shipped parameters (rna004_130bps@v1.0: 110 events, 25 kept, padding 100 -- SegParams' defaults); at least half
    the reads must succeed under the oracle, so that equality is not equality of failures"""
    for name, b in _batches():
        rows = _rows(b)
        fpt, dwell, stats, status = orc.fingerprint_batch(rows, b["a_s"], b["a_e"], orc.SegParams(barcode_num_events=K, padding=b["padding"]),
                                                          ok=b["ok"])
        # (the oracle has no window limit; the engine's documented one, WDX_MAX_ADAPTER_SAMPLES, answers status 5)
        win = np.minimum(b["a_e"].astype(np.int64) + b["padding"], rows.shape[1]) - np.maximum(b["a_s"].astype(np.int64) - b["padding"], 0)
        status = np.where((status == 0) & (win > sig_proc.MAX_ADAPTER_SAMPLES), 5, status).astype(np.int32)
        good = status == 0
        assert good.sum() * 2 >= len(status), (name, int(good.sum()), len(status))
        got = sig_proc.fingerprint_batch_adc(b["adc"], b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"], _params(b),
                                             success=b["ok"])
        assert np.array_equal(got.status, status), name
        assert np.array_equal(got.fpt[good].view(np.uint64), fpt[good].view(np.uint64)), name
        assert np.array_equal(got.dwell[good], dwell[good]) and np.array_equal(got.stats[good].view(np.uint64), stats[good].view(np.uint64)), name


def test_feeder_adc_equals_the_float32_feeder_on_a_real_model():
    """Feeder(adc=True).detect_and_predict_adc against Feeder.detect_and_predict on the calibrated rows, both on a resident
    DTW_SVM built from g6b (the reference's WDX10_rna004_v1_0 model); in a fresh interpreter whose parent never touches
    the GPU (tests/helpers/feeder_adc_check.py)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "feeder_adc_check.py")], capture_output=True,
                       text=True, cwd=ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    for name, r in rec["batches"].items():
        assert all(r["same"].values()), (name, r)
        assert r["ok_reads"] * 2 >= r["reads"] and r["pred_rows"] == r["ok_reads"], (name, r)
    assert rec["refused"] == {"float32_on_int16_ring": True, "int16_on_float32_ring": True, "short_success": True}, rec
