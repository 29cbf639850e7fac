"""Consensus refinement through the pipelined minibatches (wdx_demux_submit_refine / wdx_demux_wait_refine), the fused
device call (wdx_demux_refine_dev) and the feeder (Feeder(refine=...)).  The yardstick is always the blocking call
(`sig_proc.fingerprint_refine_batch`, which tests/test_gpu_refine.py pins to the oracle) on the same rows, followed by the
blocking DTW / DTW_SVM calls where distances and predictions are compared.  Every array bit for bit, NaN by position; no
tolerances.  Inputs: tests/helpers/refine_inputs.py (96 reads per batch, every special read asserted to occur)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import adc_inputs, refine_inputs as ri, svm_ref
from warpdemux_amd import _lib, parallel_distances as pdist, pipeline, sig_proc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (101, 202)
N_REFS, K = 16, 25
W = _lib
ALL_FP = W.WANT_FPT | W.WANT_DWELL | W.WANT_STATS | W.WANT_REFINE_IDX


def _hp(keep=K):
    return sig_proc.SegParams(barcode_num_events=keep, **ri.SEG)


def _hr(keep=K, qscale=1.0):
    return sig_proc.RefineParams(query=ri.consensus() * qscale, barcode_segm_events=25, barcode_keep_events=keep)


@functools.lru_cache(maxsize=None)
def _batch(seed):
    return ri.batch(seed)


@functools.lru_cache(maxsize=None)
def _blocking(seed, nan, keep=K, qscale=1.0):
    """THE yardstick: the blocking call on the float32 rows (computed once per variant, never modified)"""
    b = _batch(seed)
    fb = sig_proc.fingerprint_refine_batch(b["rows_nan" if nan else "rows"], b["a_s"], b["a_e"], _hp(keep), _hr(keep, qscale),
                                           success=b["ok"])
    ri.check_kinds(fb.status, nan)
    for a in (fb.fpt, fb.dwell, fb.stats, fb.status, fb.refine_idx):
        a.setflags(write=False)
    return fb


@functools.lru_cache(maxsize=None)
def _refs():
    fb = _blocking(SEEDS[0], False)
    X = np.ascontiguousarray(fb.fpt[fb.status == 0][:N_REFS])
    assert X.shape == (N_REFS, K)
    return X


@functools.lru_cache(maxsize=None)
def _dtw(seed, nan):
    """dist (n, nY) float32 with NaN rows and call (-1) for reads whose status is not 0: the blocking DTW on the blocking
    call's successful fingerprints"""
    fb = _blocking(seed, nan)
    ok = fb.status == 0
    D, am = pdist.nearest_reference(fb.fpt[ok], _refs(), 15, 0.1)
    dist = np.full((fb.status.size, N_REFS), np.nan, dtype=np.float32)
    call = np.full(fb.status.size, -1, dtype=np.int32)
    dist[ok], call[ok] = D, am
    return dist, call


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _check_fp(got, fb, what):
    for name, exp in (("status", fb.status), ("fpt", fb.fpt), ("dwell", fb.dwell), ("stats", fb.stats), ("refine_idx", fb.refine_idx)):
        if got.get(name) is not None:
            assert _same(got[name], exp), f"{what}: {name}"


class Ctx:
    """one engine context with the references resident [+ the launch chain for batches of any size]"""

    def __init__(self, chain, refs=True):
        self.L, self.ctx = _lib.load(), _lib.Context(0)
        if refs:
            X = _refs()
            _lib.check(self.L.wdx_set_refs(self.ctx.handle, _lib.ptr(X), N_REFS, K, 15, 0.1))
        if chain:
            self.ctx.set_option(_lib.OPT_FAST_CHAIN_MIN_READS, 1)

    def submit(self, slot, desc, hp, hr, n_refs, want):
        pc, rc = hp.to_c(), hr.to_c()
        f, a = (C.byref(desc), None) if isinstance(desc, _lib.MinibatchInC) else (None, C.byref(desc))
        return self.L.wdx_demux_submit_refine(self.ctx.handle, slot, f, a, C.byref(pc), C.byref(rc), n_refs, want)

    def wait(self, slot, n, want, keep=K, k=0, ridx="auto", ex=False):
        o = dict(status=np.full(n, -9, np.int32), call=np.full(n, -9, np.int32),
                 dist=np.empty((n, N_REFS), np.float32) if want & W.WANT_DIST else None,
                 fpt=np.empty((n, keep)) if want & W.WANT_FPT else None,
                 dwell=np.empty((n, keep), np.int64) if want & W.WANT_DWELL else None,
                 stats=np.empty((n, 6)) if want & W.WANT_STATS else None,
                 prob=np.empty((n, k)) if want & W.WANT_SVM else None, pred=np.empty(n, np.int32) if want & W.WANT_SVM else None,
                 conf=np.empty(n) if want & W.WANT_SVM else None)
        out = _lib.MinibatchOutC(*[_lib.addr(o[key]) for key in ("status", "call", "dist", "fpt", "dwell", "stats", "prob", "pred", "conf")])
        if ridx == "auto":
            ridx = bool(want & W.WANT_REFINE_IDX)
        o["refine_idx"] = np.empty((n, 3), np.int32) if ridx else None
        if ex:
            return self.L.wdx_demux_wait_ex(self.ctx.handle, slot, C.byref(out)), o
        return self.L.wdx_demux_wait_refine(self.ctx.handle, slot, C.byref(out), _lib.ptr(o["refine_idx"])), o

    def close(self):
        self.ctx.close()


def _float_ways(b, rows):
    """the three ways in of float32 rows -> {name: (descriptor, arrays kept alive)}"""
    n, stride = rows.shape
    pinned = pipeline.pinned_empty(rows.shape, np.float32)
    pinned[:] = rows
    flat, off, rlen, a_s2, a_e2 = ri.pack_rows_f32(b, rows)
    mk = _lib.MinibatchInC
    return {
        "pageable": (mk(_lib.addr(rows), n, stride, None, None, _lib.addr(b["a_s"]), _lib.addr(b["a_e"]), _lib.addr(b["ok"])), rows),
        "page-locked": (mk(_lib.addr(pinned), n, stride, None, None, _lib.addr(b["a_s"]), _lib.addr(b["a_e"]), _lib.addr(b["ok"])), pinned),
        "packed": (mk(_lib.addr(flat), n, 0, _lib.addr(off), _lib.addr(rlen), _lib.addr(a_s2), _lib.addr(a_e2), _lib.addr(b["ok"])),
                   (flat, off, rlen, a_s2, a_e2)),
    }


def _adc_ways(b):
    cal = (b["row_len"], b["offset"], b["scale"])
    pinned = pipeline.pinned_empty(b["adc"].shape, np.int16)
    pinned[:] = b["adc"]
    flat, off, rlen, rwin, a_s2, a_e2 = adc_inputs.pack_rows(b)
    ways = {
        "pageable": sig_proc.adc_minibatch(b["adc"], *cal, b["a_s"], b["a_e"], b["ok"]),
        "page-locked": sig_proc.adc_minibatch(pinned, *cal, b["a_s"], b["a_e"], b["ok"]),
        "packed": sig_proc.adc_minibatch(flat, rlen, b["offset"], b["scale"], a_s2, a_e2, b["ok"], row_off=off, row_win=rwin),
    }
    return {name: (v[0], v[2]) for name, v in ways.items()}


def _three_ways(ways, fb, dtw, chain, what):
    n = fb.status.size
    c = Ctx(chain)
    try:
        for name, (desc, _keep) in ways.items():
            want = ALL_FP | W.WANT_DIST
            assert c.submit(0, desc, _hp(), _hr(), N_REFS, want) == 0, c.L.wdx_last_error()
            rc, got = c.wait(0, n, want)
            assert rc == 0, c.L.wdx_last_error()
            _check_fp(got, fb, f"{what} {name}")
            assert _same(got["dist"], dtw[0]) and _same(got["call"], dtw[1]), f"{what} {name}: dist / call"
            # fingerprint only: no references asked for, FPT | REFINE_IDX
            want = W.WANT_FPT | W.WANT_REFINE_IDX
            assert c.submit(1, desc, _hp(), _hr(), 0, want) == 0, c.L.wdx_last_error()
            rc, got = c.wait(1, n, want)
            assert rc == 0, c.L.wdx_last_error()
            _check_fp(got, fb, f"{what} {name} n_refs=0")
            assert (got["call"] == -1).all()
    finally:
        c.close()


@pytest.mark.parametrize("chain", [False, True], ids=["as-is", "launch-chain"])
@pytest.mark.parametrize("seed", SEEDS)
def test_submit_refine_float32_rows_three_ways_in(seed, chain):
    b = _batch(seed)
    _three_ways(_float_ways(b, b["rows_nan"]), _blocking(seed, True), _dtw(seed, True), chain, "float32")


@pytest.mark.parametrize("chain", [False, True], ids=["as-is", "launch-chain"])
@pytest.mark.parametrize("seed", SEEDS)
def test_submit_refine_int16_rows_three_ways_in(seed, chain):
    """the int16 rows against the blocking call on `calibrate_adc` of them (int16 holds no NaN: the NaN tail is the one
    kind of NaN window here)"""
    b = _batch(seed)
    assert _same(sig_proc.calibrate_adc(b["adc"], b["row_len"], b["offset"], b["scale"]), b["rows"])
    _three_ways(_adc_ways(b), _blocking(seed, False), _dtw(seed, False), chain, "int16")


@pytest.mark.parametrize("chain", [False, True], ids=["as-is", "launch-chain"])
def test_two_slots_in_flight_with_different_refinement_parameters(chain):
    """slot 0: the tRNA set against the references; slot 1: 20 events kept, the query scaled by 1.01, fingerprints only
    -- submitted back to back, waited for in the other order; each gets its own answer"""
    b = _batch(SEEDS[1])
    n = b["rows"].shape[0]
    fa, fb2 = _blocking(SEEDS[1], False), _blocking(SEEDS[1], False, 20, 1.01)
    assert not _same(fa.refine_idx, fb2.refine_idx) or not _same(fa.stats, fb2.stats) or fa.fpt.shape != fb2.fpt.shape
    ways = _float_ways(b, b["rows"])
    c = Ctx(chain)
    try:
        assert c.submit(0, ways["pageable"][0], _hp(), _hr(), N_REFS, ALL_FP | W.WANT_DIST) == 0, c.L.wdx_last_error()
        assert c.submit(1, ways["page-locked"][0], _hp(20), _hr(20, 1.01), 0, ALL_FP) == 0, c.L.wdx_last_error()
        rc1, g1 = c.wait(1, n, ALL_FP, keep=20)
        rc0, g0 = c.wait(0, n, ALL_FP | W.WANT_DIST)
        assert rc0 == 0 and rc1 == 0, c.L.wdx_last_error()
        _check_fp(g0, fa, "slot 0")
        _check_fp(g1, fb2, "slot 1")
        assert _same(g0["dist"], _dtw(SEEDS[1], False)[0]) and _same(g0["call"], _dtw(SEEDS[1], False)[1])
        assert (g1["call"] == -1).all()
    finally:
        c.close()


@pytest.mark.parametrize("chain", [False, True], ids=["as-is", "launch-chain"])
def test_demux_refine_dev_is_blocking_refine_then_dtw_then_argmin(chain):
    import torch

    from warpdemux_amd.engine import DemuxEngine

    seed = SEEDS[0]
    b, fb = _batch(seed), _blocking(seed, True)
    rows = b["rows_nan"]
    n, stride = rows.shape
    eng = DemuxEngine(_refs(), 15, 0.1, _hp())
    d = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731  (a copy: the yardstick's arrays are read-only)
    try:
        if chain:
            eng.ctx.set_option(_lib.OPT_FAST_CHAIN_MIN_READS, 1)
        # the yardstick's second half: wdx_dtw_matrix_dev on the blocking call's fingerprints, then the argmin
        dist_t, am_t = eng.dtw(d(fb.fpt))
        torch.cuda.synchronize()
        dist, am = dist_t.cpu().numpy(), am_t.cpu().numpy()
        ok = fb.status == 0
        call = np.where(ok, am, -1).astype(np.int32)
        counts = np.bincount(call[ok], minlength=N_REFS + 1).astype(np.int64)
        counts[N_REFS] = (~ok).sum()
        assert counts[N_REFS] >= 5 and (fb.status == 6).sum() >= 3
        flat, off, rlen, a_s2, a_e2 = ri.pack_rows_f32(b, rows)
        for layout in ("minibatch", "packed"):
            if layout == "minibatch":
                res, dwell, stats, idx = eng.demux_refine(d(rows), d(b["a_s"]), d(b["a_e"]), _hr(), stride=stride, max_len=stride,
                                                          ok=d(b["ok"]))
            else:
                res, dwell, stats, idx = eng.demux_refine(d(flat), d(a_s2), d(a_e2), _hr(), offsets=d(off), max_len=int(rlen.max()),
                                                          ok=d(b["ok"]))
            torch.cuda.synchronize()
            got = dict(status=res.status.cpu().numpy(), fpt=res.fpt.cpu().numpy(), dwell=dwell.cpu().numpy(),
                       stats=stats.cpu().numpy(), refine_idx=idx.cpu().numpy())
            _check_fp(got, fb, layout)
            assert _same(res.call.cpu().numpy(), call), layout
            got_dist = res.dist.cpu().numpy()
            assert _same(got_dist[ok], dist[ok]) and np.isnan(got_dist[~ok]).all(), layout   # (failed reads: NaN rows)
            assert _same(res.counts.cpu().numpy(), counts), layout
    finally:
        eng.close()


@pytest.mark.parametrize("chain", [False, True], ids=["as-is", "launch-chain"])
def test_want_svm_on_refine_minibatches(chain):
    """WDX_WANT_SVM: prob / pred / conf of the successful reads = wdx_dtw_svm_predict on their blocking fingerprints;
    every other read, consensus outliers included, pred -1 and NaN"""
    seed = SEEDS[1]
    b, fb = _batch(seed), _blocking(seed, True)
    n = fb.status.size
    ok = fb.status == 0
    m = svm_ref.synth_model(3, seed=3, n_support=[4, 3, 5], n_extra=N_REFS - 12, thresholds=True, pwr_dist=2)
    D = _dtw(seed, True)[0][ok]
    m.gamma = float(np.float32(1.5 / float(np.median(D)) ** 2))     # median kernel value ~ exp(-1.5)
    model = m.to_dtw_svm(_refs())
    c = Ctx(chain)
    try:
        mc = model.to_c()
        _lib.check(c.L.wdx_svm_set_model(c.ctx.handle, C.byref(mc)))
        X = np.ascontiguousarray(fb.fpt[ok])
        prob, pred, conf = np.empty((X.shape[0], m.k)), np.empty(X.shape[0], np.int32), np.empty(X.shape[0])
        _lib.check(c.L.wdx_dtw_svm_predict(c.ctx.handle, _lib.ptr(X), X.shape[0], _lib.ptr(prob), _lib.ptr(pred), _lib.ptr(conf)))
        assert np.ptp(prob, axis=0).min() > 0 and (pred >= 0).any()
        e_prob, e_pred, e_conf = np.full((n, m.k), np.nan), np.full(n, -1, np.int32), np.full(n, np.nan)
        e_prob[ok], e_pred[ok], e_conf[ok] = prob, pred, conf
        want = ALL_FP | W.WANT_DIST | W.WANT_SVM
        for name, (desc, _keep) in _float_ways(b, b["rows_nan"]).items():
            assert c.submit(0, desc, _hp(), _hr(), N_REFS, want) == 0, c.L.wdx_last_error()
            rc, got = c.wait(0, n, want, k=m.k)
            assert rc == 0, c.L.wdx_last_error()
            _check_fp(got, fb, name)
            assert _same(got["prob"], e_prob) and _same(got["pred"], e_pred) and _same(got["conf"], e_conf), name
            six = fb.status == 6
            assert six.sum() >= 3 and (got["pred"][six] == -1).all() and np.isnan(got["prob"][six]).all()
    finally:
        c.close()


def test_errors_leave_the_slot_as_wait_ex_does():
    seed = SEEDS[0]
    b, fb = _batch(seed), _blocking(seed, False)
    n = fb.status.size
    desc = _float_ways(b, b["rows"])["pageable"][0]
    c = Ctx(False)
    INV = _lib.WDX_ERR_INVALID
    try:
        # K != reference length; distances without references: refused, nothing in the slot
        assert c.submit(0, desc, _hp(20), _hr(20), N_REFS, ALL_FP) == INV
        assert c.submit(0, desc, _hp(), _hr(), 0, ALL_FP | W.WANT_DIST) == INV
        assert c.submit(0, desc, _hp(), _hr(), 0, ALL_FP | W.WANT_SVM) == INV
        assert c.submit(0, desc, _hp(), _hr(), N_REFS + 1, ALL_FP) == INV
        assert c.wait(0, n, 0)[0] == INV, "nothing was submitted"
        # refine_idx not asked for, but passed: refused, the slot stays busy, a correct wait then succeeds
        want = W.WANT_FPT
        assert c.submit(0, desc, _hp(), _hr(), N_REFS, want) == 0, c.L.wdx_last_error()
        assert c.wait(0, n, want, ridx=True)[0] == INV
        assert c.submit(0, desc, _hp(), _hr(), N_REFS, want) == INV, "the slot is still busy"
        rc, got = c.wait(0, n, want, ex=True)            # wdx_demux_wait_ex completes a refine slot without refine_idx
        assert rc == 0, c.L.wdx_last_error()
        _check_fp(got, fb, "after a refused wait")
        assert _same(got["call"], _dtw(seed, False)[1])
        # refine_idx asked for: wdx_demux_wait_ex (and a wait without the pointer) refuse, the right wait succeeds
        assert c.submit(0, desc, _hp(), _hr(), N_REFS, ALL_FP) == 0, c.L.wdx_last_error()
        assert c.wait(0, n, ALL_FP, ex=True)[0] == INV
        assert c.wait(0, n, ALL_FP, ridx=False)[0] == INV
        rc, got = c.wait(0, n, ALL_FP)
        assert rc == 0, c.L.wdx_last_error()
        _check_fp(got, fb, "after wait_ex was refused")
        assert got["refine_idx"] is not None and c.wait(0, n, 0)[0] == INV, "the slot is free again"
    finally:
        c.close()


def test_python_pipeline_with_refine():
    """MinibatchPipeline(refine=...): float32 and int16 minibatches through `run`, and a fingerprint-only pipeline"""
    b = _batch(SEEDS[0])
    fb, fbn = _blocking(SEEDS[0], False), _blocking(SEEDS[0], True)
    dist, call = _dtw(SEEDS[0], False)
    pipe = pipeline.MinibatchPipeline(_refs(), 15, 0.1, _hp(), refine=_hr())
    try:
        mbs = [(b["rows_nan"], b["a_s"], b["a_e"], b["ok"]),
               (b["adc"], b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"], b["ok"]),
               (b["rows"], b["a_s"], b["a_e"], b["ok"])]
        res = list(pipe.run(mbs))
    finally:
        pipe.close()
    for r, want in zip(res, (fbn, fb, fb)):
        _check_fp(vars(r.fingerprints), want, "pipeline")
    assert _same(res[1].dist, dist) and _same(res[1].call, call) and _same(res[2].dist, dist)
    solo = pipeline.MinibatchPipeline(None, params=_hp(), refine=_hr())
    try:
        solo.submit(0, b["rows"], b["a_s"], b["a_e"], b["ok"])
        r = solo.wait(0)
    finally:
        solo.close()
    _check_fp(vars(r.fingerprints), fb, "fingerprint-only pipeline")
    assert r.dist is None and (r.call == -1).all()


def test_feeder_with_refine_forked_workers():
    """Feeder(refine=...) from four forked workers (float32 rows, then int16 rows), a fingerprint-only feeder without
    references and a plain Feeder beside them, in a fresh interpreter whose parent process never touches the GPU
    (tests/helpers/feeder_refine_check.py)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "feeder_refine_check.py")], capture_output=True,
                       text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["gpu_processes"] <= 6
    for run in ("float32", "int16", "fingerprint_only", "plain"):
        assert rec[run] and all(rec[run].values()), (run, rec[run])
    assert rec["kinds_ok"] and rec["refused"] == {"demux_on_fingerprint_only": True, "predict_without_model": True}
