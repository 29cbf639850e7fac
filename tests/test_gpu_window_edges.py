"""The adapter windows at the edges of their rows, through every host way in of float32 rows: the 2-D copy of a pageable
batch, the window pack of a page-locked one, rows the caller packed, and a feeder worker.  Accepted detections (ok = 1)
whose window starts at the row's end, one and five samples beyond it (the last row of the batch among them), an inverted
window and a window clipped at both ends must come out of all four ways exactly as out of the pageable one -- status, fpt
and call bit for bit -- and the pageable run must equal the CPU oracle on the unpacked rows.  That no way in addresses a
sample outside its row is proven on the CPU (tests/test_window_host.py); here the page-locked and the feeder batch simply
end with their last row."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import window_inputs as wi
from oracle import wdx_oracle as orc
from warpdemux_amd import _lib, pipeline, sig_proc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = _lib.WANT_FPT


@functools.lru_cache(maxsize=None)
def _inputs():
    b = wi.batch()
    fpt, status, refs = wi.oracle(b)
    for a in (b["rows"], b["a_s"], b["a_e"], b["ok"], fpt, status, refs):
        a.setflags(write=False)
    return b, fpt, status, refs


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_the_batch_holds_its_edges_and_takes_both_float32_branches():
    b, _fpt, status, _refs = _inputs()
    start = b["a_s"].astype(np.int64) - wi.PADDING
    assert start[wi.I_AT] == wi.STRIDE and start[wi.I_PLUS1] == wi.STRIDE + 1 and start[wi.I_PLUS5] == wi.STRIDE + 5
    assert wi.I_PLUS5 == wi.N - 1 and b["a_e"][wi.I_INVERTED] < b["a_s"][wi.I_INVERTED] and b["ok"].all()
    assert start[wi.I_CLIPPED] < 0 and b["a_e"][wi.I_CLIPPED] + wi.PADDING > wi.STRIDE
    # below 0.85 a page-locked batch is packed over the bus; a pageable one always takes the 2-D copy
    assert wi.windows_to_box_ratio(b) < 0.8
    edges = [wi.I_AT, wi.I_PLUS1, wi.I_PLUS5, wi.I_INVERTED]
    assert (status[edges] != 0).all() and status[wi.I_CLIPPED] == 0 and (status == 0).sum() == wi.N - len(edges)


@functools.lru_cache(maxsize=None)
def _three_ways():
    """{way: (status, fpt, call)} of one context with the references resident"""
    b, _fpt, _status, refs = _inputs()
    rows, n = b["rows"], wi.N
    pinned = pipeline.pinned_empty((wi.N, wi.STRIDE), np.float32)      # exactly N * STRIDE floats: no slack behind the last row
    pinned[:] = rows
    flat, off, rlen, a_s2, a_e2 = wi.pack_rows(b)
    a_s, a_e, ok = (_lib.addr(b[k]) for k in ("a_s", "a_e", "ok"))
    ways = {
        "pageable": _lib.MinibatchInC(_lib.addr(rows), n, wi.STRIDE, None, None, a_s, a_e, ok),
        "page-locked": _lib.MinibatchInC(_lib.addr(pinned), n, wi.STRIDE, None, None, a_s, a_e, ok),
        "packed": _lib.MinibatchInC(_lib.addr(flat), n, 0, _lib.addr(off), _lib.addr(rlen), _lib.addr(a_s2), _lib.addr(a_e2), ok),
    }
    L, ctx = _lib.load(), _lib.Context(0)
    pc = sig_proc.SegParams(**wi.SEG).to_c()
    got = {}
    try:
        _lib.check(L.wdx_set_refs(ctx.handle, _lib.ptr(refs), wi.N_REFS, wi.K, 15, 0.1))
        for name, desc in ways.items():
            status, call, fpt = np.full(n, -9, np.int32), np.full(n, -9, np.int32), np.empty((n, wi.K))
            _lib.check(L.wdx_demux_submit_ex(ctx.handle, 0, C.byref(desc), C.byref(pc), wi.N_REFS, WANT))
            out = _lib.MinibatchOutC(_lib.addr(status), _lib.addr(call), None, _lib.addr(fpt), None, None, None, None, None)
            _lib.check(L.wdx_demux_wait_ex(ctx.handle, 0, C.byref(out)))
            got[name] = (status, fpt, call)
    finally:
        ctx.close()
    return got


def test_pageable_run_equals_the_oracle():
    b, fpt, status, refs = _inputs()
    g_status, g_fpt, g_call = _three_ways()["pageable"]
    assert _same(g_status, status)
    good = status == 0
    assert np.array_equal(g_fpt[good].view(np.uint64), fpt[good].view(np.uint64)) and np.isnan(g_fpt[~good]).all()
    want_call = np.full(wi.N, -1, np.int32)
    want_call[good] = np.argmin(orc.dtw_matrix(fpt[good], refs, 15, 0.1), axis=1)
    assert _same(g_call, want_call)
    # the blocking fingerprint call shares the pageable way's staging
    fb = sig_proc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], sig_proc.SegParams(**wi.SEG), success=b["ok"])
    assert _same(fb.status, g_status) and _same(fb.fpt, g_fpt)


@pytest.mark.parametrize("way", ["page-locked", "packed"])
def test_every_way_in_equals_the_pageable_run(way):
    got, ref = _three_ways()[way], _three_ways()["pageable"]
    for name, a, e in zip(("status", "fpt", "call"), got, ref):
        assert _same(a, e), f"{way}: {name}"


def test_feeder_worker_equals_the_pageable_run(tmp_path):
    out = str(tmp_path / "feeder.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "feeder_window_check.py"), out],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = np.load(out)
    status, fpt, call = _three_ways()["pageable"]
    assert _same(got["status"], status) and _same(got["demux_status"], status)
    assert _same(got["fpt"], fpt) and _same(got["call"], call)
