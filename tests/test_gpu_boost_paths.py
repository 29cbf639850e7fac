"""The Fpt_Boost tail on host-fed minibatches: WDX_WANT_BOOST through wdx_demux_submit_ex / _adc / _refine,
`MinibatchPipeline(model=...)` and `Feeder(model=...)`.  The yardstick is always the blocking fingerprint call
(`sig_proc.fingerprint_batch` / `fingerprint_refine_batch`) followed by `wdx_boost_predict` on the successful fingerprints
(`Fpt_Boost.predict_raw`); failed reads carry pred -1 and NaN.  Every array bit for bit, NaN by position; no tolerances.
Inputs: tests/helpers/refine_inputs.py (96 reads, failed reads and consensus outliers among them), in float32 and int16."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import adc_inputs, boost_ref, refine_inputs as ri
from warpdemux_amd import _lib, models, parallel_distances as pdist, pipeline, sig_proc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, N_REFS, K = 101, 16, 25
W = _lib
FP = W.WANT_FPT | W.WANT_DWELL | W.WANT_STATS
INV, NO_REFS = _lib.WDX_ERR_INVALID, _lib.WDX_ERR_NO_REFS
THR = np.array([0.05, 0.2, 0.1, 0.3])


def _hp(keep=K):
    return sig_proc.SegParams(barcode_num_events=keep, **ri.SEG)


def _hr(keep=K):
    return sig_proc.RefineParams(query=ri.consensus(), barcode_segm_events=25, barcode_keep_events=keep)


@functools.lru_cache(maxsize=None)
def _batch():
    return ri.batch(SEED)


@functools.lru_cache(maxsize=None)
def _model(n_features=K):
    """the device model (and its restatement): fingerprints are normalised event means, the borders cut through them"""
    m = boost_ref.random_model(65, 6, 4, n_features, seed=81)
    trees = [(f, b, [False] * len(f), lv) for f, b, lv in m.trees]
    return models.Fpt_Boost(trees, m.n_features, m.scale, m.bias, {0: 7, 1: 1, 2: 10, 3: 4}, THR), m


@functools.lru_cache(maxsize=None)
def _yard(refine, nan):
    """THE yardstick: the blocking fingerprint call, then wdx_boost_predict on the successful rows (computed once)"""
    b = _batch()
    rows = b["rows_nan" if nan else "rows"]
    fb = (sig_proc.fingerprint_refine_batch(rows, b["a_s"], b["a_e"], _hp(), _hr(), success=b["ok"]) if refine
          else sig_proc.fingerprint_batch(rows, b["a_s"], b["a_e"], _hp(), success=b["ok"]))
    ok = fb.status == 0
    n = ok.size
    assert 40 <= ok.sum() < n and fb.status[ri.I_DEAD] == 1 and fb.status[ri.I_SHORT] == 3
    if refine:
        ri.check_kinds(fb.status, nan)
    dm, m = _model()
    raw, prob, pred, conf = dm.predict_raw(fb.fpt[ok])
    assert np.array_equal(raw, boost_ref.raw_scores(m, fb.fpt[ok])) and len(set(pred.tolist())) >= 3
    e = dict(prob=np.full((n, 4), np.nan), pred=np.full(n, -1, np.int32), conf=np.full(n, np.nan))
    e["prob"][ok], e["pred"][ok], e["conf"][ok] = prob, pred.astype(np.int32), conf
    e.update(status=fb.status, fpt=fb.fpt, dwell=fb.dwell, stats=fb.stats, refine_idx=fb.refine_idx)
    for a in e.values():
        if a is not None:
            a.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def _refs(refine):
    e = _yard(refine, False)
    return np.ascontiguousarray(e["fpt"][e["status"] == 0][:N_REFS])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _check(got, e, what):
    for name in ("status", "fpt", "dwell", "stats", "refine_idx", "prob", "pred", "conf"):
        if got.get(name) is not None:
            assert _same(got[name], e[name]), f"{what}: {name}"
    bad = e["status"] != 0
    assert (got["pred"][bad] == -1).all() and np.isnan(got["prob"][bad]).all() and np.isnan(got["conf"][bad]).all(), what


class Ctx:
    """one engine context [+ references] [+ the boost model]"""

    def __init__(self, refs=None, model=True):
        self.L, self.ctx = _lib.load(), _lib.Context(0)
        if refs is not None:
            _lib.check(self.L.wdx_set_refs(self.ctx.handle, _lib.ptr(refs), N_REFS, K, 15, 0.1))
        if model:
            self.set_model(_model()[0])

    def set_model(self, dm):
        mc = dm.to_c()
        _lib.check(self.L.wdx_boost_set_model(self.ctx.handle, C.byref(mc)))

    def submit(self, slot, desc, n_refs, want, refine=False, keep=K):
        pc = _hp(keep).to_c()
        adc = isinstance(desc, _lib.MinibatchAdcInC)
        if refine:
            rc = _hr(keep).to_c()
            return self.L.wdx_demux_submit_refine(self.ctx.handle, slot, None if adc else C.byref(desc),
                                                  C.byref(desc) if adc else None, C.byref(pc), C.byref(rc), n_refs, want)
        call = self.L.wdx_demux_submit_adc if adc else self.L.wdx_demux_submit_ex
        return call(self.ctx.handle, slot, C.byref(desc), C.byref(pc), n_refs, want)

    def wait(self, slot, n, want, tail=None, ex=False):
        tail = bool(want & (W.WANT_SVM | W.WANT_BOOST)) if tail is None else tail
        o = dict(status=np.full(n, -9, np.int32), call=np.full(n, -9, np.int32),
                 dist=np.empty((n, N_REFS), np.float32) if want & W.WANT_DIST else None,
                 fpt=np.empty((n, K)) if want & W.WANT_FPT else None,
                 dwell=np.empty((n, K), np.int64) if want & W.WANT_DWELL else None,
                 stats=np.empty((n, 6)) if want & W.WANT_STATS else None,
                 prob=np.empty((n, 4)) if tail else None, pred=np.empty(n, np.int32) if tail else None,
                 conf=np.empty(n) if tail else None)
        out = _lib.MinibatchOutC(*[_lib.addr(o[key]) for key in ("status", "call", "dist", "fpt", "dwell", "stats", "prob", "pred", "conf")])
        o["refine_idx"] = np.empty((n, 3), np.int32) if want & W.WANT_REFINE_IDX else None
        if ex:
            return self.L.wdx_demux_wait_ex(self.ctx.handle, slot, C.byref(out)), o
        return self.L.wdx_demux_wait_refine(self.ctx.handle, slot, C.byref(out), _lib.ptr(o["refine_idx"])), o

    def close(self):
        self.ctx.close()


@functools.lru_cache(maxsize=None)
def _ways(fmt):
    """the three ways in of float32 rows (with a NaN inside a window) / int16 rows -> {name: (descriptor, kept alive)}"""
    b = _batch()
    if fmt == "int16":
        cal = (b["row_len"], b["offset"], b["scale"])
        pinned = pipeline.pinned_empty(b["adc"].shape, np.int16)
        pinned[:] = b["adc"]
        flat, off, rlen, rwin, a_s2, a_e2 = adc_inputs.pack_rows(b)
        ways = {"pageable": sig_proc.adc_minibatch(b["adc"], *cal, b["a_s"], b["a_e"], b["ok"]),
                "page-locked": sig_proc.adc_minibatch(pinned, *cal, b["a_s"], b["a_e"], b["ok"]),
                "packed": sig_proc.adc_minibatch(flat, rlen, b["offset"], b["scale"], a_s2, a_e2, b["ok"], row_off=off, row_win=rwin)}
        return {name: (v[0], v[2]) for name, v in ways.items()}
    rows = b["rows_nan"]
    n, stride = rows.shape
    pinned = pipeline.pinned_empty(rows.shape, np.float32)
    pinned[:] = rows
    flat, off, rlen, a_s2, a_e2 = ri.pack_rows_f32(b, rows)
    mk, ad = _lib.MinibatchInC, _lib.addr
    return {"pageable": (mk(ad(rows), n, stride, None, None, ad(b["a_s"]), ad(b["a_e"]), ad(b["ok"])), rows),
            "page-locked": (mk(ad(pinned), n, stride, None, None, ad(b["a_s"]), ad(b["a_e"]), ad(b["ok"])), pinned),
            "packed": (mk(ad(flat), n, 0, ad(off), ad(rlen), ad(a_s2), ad(a_e2), ad(b["ok"])), (flat, off, rlen, a_s2, a_e2))}


@pytest.mark.parametrize("kernel", [1, 2], ids=["lane-per-read", "tree-parallel"])
@pytest.mark.parametrize("refine", [False, True], ids=["plain", "refine"])
@pytest.mark.parametrize("fmt", ["float32", "int16"])
def test_want_boost_without_references_three_ways_in(fmt, refine, kernel):
    """n_refs == 0: no reference set on the context at all; call is -1 everywhere"""
    e = _yard(refine, fmt == "float32")
    n = e["status"].size
    want = FP | W.WANT_BOOST | (W.WANT_REFINE_IDX if refine else 0)
    c = Ctx()
    try:
        c.ctx.set_option(_lib.OPT_BOOST_KERNEL, kernel)
        for name, (desc, _keep) in _ways(fmt).items():
            assert c.submit(0, desc, 0, want, refine) == 0, c.L.wdx_last_error()
            rc, got = c.wait(0, n, want)
            assert rc == 0, c.L.wdx_last_error()
            _check(got, e, f"{fmt} {name}")
            assert (got["call"] == -1).all()
    finally:
        c.close()


@pytest.mark.parametrize("refine", [False, True], ids=["plain", "refine"])
def test_want_boost_beside_the_dtw_against_resident_references(refine):
    """n_refs = nY with WDX_WANT_DIST: call and dist are those of the blocking DTW path (plain: wdx_demux_batch), the boost
    tail runs beside them"""
    b = _batch()
    refs = _refs(refine)
    if refine:
        e = _yard(True, False)
        ok = e["status"] == 0
        D, am = pdist.nearest_reference(e["fpt"][ok], refs, 15, 0.1)
        dist, call = np.full((ok.size, N_REFS), np.nan, np.float32), np.full(ok.size, -1, np.int32)
        dist[ok], call[ok] = D, am
    else:
        sig_proc.set_references(refs, 15, 0.1)
        db = sig_proc.demux_batch(b["rows"], b["a_s"], b["a_e"], _hp(), success=b["ok"], want_dist=True)
        dist, call = db.dist, db.call
        assert _same(db.status, _yard(False, False)["status"])
    n = call.size
    want = FP | W.WANT_BOOST | W.WANT_DIST | (W.WANT_REFINE_IDX if refine else 0)
    c = Ctx(refs)
    try:
        for fmt in ("float32", "int16"):
            e = _yard(refine, False)
            desc = _ways("int16")["pageable"][0] if fmt == "int16" else _lib.MinibatchInC(
                _lib.addr(b["rows"]), n, b["rows"].shape[1], None, None, _lib.addr(b["a_s"]), _lib.addr(b["a_e"]), _lib.addr(b["ok"]))
            assert c.submit(0, desc, N_REFS, want, refine) == 0, c.L.wdx_last_error()
            rc, got = c.wait(0, n, want)
            assert rc == 0, c.L.wdx_last_error()
            _check(got, e, fmt)
            assert _same(got["dist"], dist) and _same(got["call"], call), fmt
    finally:
        c.close()


def test_two_slots_in_flight_and_a_model_change_between_submits():
    """slot 0 plain, slot 1 refine, waited for in the other order; a model set afterwards answers the next submit and
    leaves what was in flight with the answers of the model it was submitted with"""
    ep, er = _yard(False, True), _yard(True, True)
    n = ep["status"].size
    ways = _ways("float32")
    wp, wr = FP | W.WANT_BOOST, FP | W.WANT_BOOST | W.WANT_REFINE_IDX
    c = Ctx()
    try:
        assert c.submit(0, ways["pageable"][0], 0, wp, False) == 0, c.L.wdx_last_error()
        assert c.submit(1, ways["page-locked"][0], 0, wr, True) == 0, c.L.wdx_last_error()
        dm, m = _model()
        m2 = boost_ref.random_model(7, 3, 4, K, seed=82)
        dm2 = models.Fpt_Boost([(f, b_, [False] * len(f), lv) for f, b_, lv in m2.trees], K, m2.scale, m2.bias,
                               {i: i for i in range(4)})
        c.set_model(dm2)
        rc1, g1 = c.wait(1, n, wr)
        rc0, g0 = c.wait(0, n, wp)
        assert rc0 == 0 and rc1 == 0, c.L.wdx_last_error()
        _check(g0, ep, "slot 0")
        _check(g1, er, "slot 1")
        assert c.submit(0, ways["packed"][0], 0, wp, False) == 0, c.L.wdx_last_error()
        rc, g2 = c.wait(0, n, wp)
        assert rc == 0
        ok = ep["status"] == 0
        _, prob2, pred2, conf2 = dm2.predict_raw(ep["fpt"][ok])
        assert _same(g2["fpt"], ep["fpt"]) and not _same(g2["prob"], ep["prob"])
        assert _same(g2["prob"][ok], prob2) and _same(g2["pred"][ok], pred2.astype(np.int32)) and _same(g2["conf"][ok], conf2)
        _model()[0]._ensure_resident()                          # (the yardstick's own context gets its model back)
    finally:
        c.close()


def test_refusals_leave_the_slot_reusable():
    e = _yard(False, True)
    n = e["status"].size
    f32, i16 = _ways("float32")["pageable"][0], _ways("int16")["pageable"][0]
    want = FP | W.WANT_BOOST
    bare = Ctx(model=False)
    try:
        # no boost model resident: the code WDX_WANT_SVM answers without an SVM; n_refs == 0 without the bit: as ever
        for desc in (f32, i16):
            assert bare.submit(0, desc, 0, want) == NO_REFS
            assert bare.submit(0, desc, 0, want, refine=True) == NO_REFS
            assert bare.submit(0, desc, 0, FP) == NO_REFS
        assert bare.submit(0, f32, 0, FP | W.WANT_SVM | W.WANT_BOOST) == INV
        bare.set_model(_model()[0])
        assert bare.submit(0, f32, 0, want) == 0, "every refusal left the slot free"
        assert bare.wait(0, n, want)[0] == 0
    finally:
        bare.close()
    c = Ctx(_refs(False))
    try:
        for desc in (f32, i16):
            for refine in (False, True):
                assert c.submit(0, desc, 0, want | W.WANT_SVM, refine) == INV
                assert c.submit(0, desc, N_REFS, want | W.WANT_SVM, refine) == INV
                assert c.submit(0, desc, 0, want | W.WANT_DIST, refine) == INV          # no references, no distances
                assert c.submit(0, desc, 0, want, refine, keep=20) == INV                # K != the model's features
                assert c.submit(0, desc, N_REFS + 1, want, refine) == INV                # not the resident nY
            assert c.submit(0, desc, 0, FP) == INV                                       # n_refs == 0 needs the bit
        c.set_model(_model(20)[0])
        assert c.submit(0, f32, N_REFS, want) == INV and c.submit(0, f32, 0, want) == INV
        assert b"boost model's features (20)" in c.L.wdx_last_error()
        c.set_model(_model()[0])
        assert c.wait(0, n, 0)[0] == INV, "nothing was submitted"
        # prob / pred / conf from a slot that asked for neither tail: refused, the slot stays busy, the right wait succeeds
        assert c.submit(0, f32, N_REFS, FP) == 0, c.L.wdx_last_error()
        assert c.wait(0, n, FP, tail=True)[0] == INV
        assert c.submit(0, f32, 0, want) == INV, "the slot is still busy"
        rc, got = c.wait(0, n, FP, ex=True)
        assert rc == 0 and _same(got["fpt"], e["fpt"])
        # ... and a slot that asked for the boost tail hands it over through either wait
        assert c.submit(0, f32, 0, want) == 0, c.L.wdx_last_error()
        rc, got = c.wait(0, n, want, ex=True)
        assert rc == 0, c.L.wdx_last_error()
        _check(got, e, "after the refusals")
    finally:
        c.close()


@pytest.mark.parametrize("refine", [False, True], ids=["plain", "refine"])
def test_python_pipeline_with_a_boost_model(refine):
    """MinibatchPipeline(refs=None, model=...): float32 and int16 minibatches through `run`"""
    b = _batch()
    en, e = _yard(refine, True), _yard(refine, False)
    pipe = pipeline.MinibatchPipeline(None, params=_hp(), model=_model()[0], refine=_hr() if refine else None)
    try:
        mbs = [(b["rows_nan"], b["a_s"], b["a_e"], b["ok"]),
               (b["adc"], b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"], b["ok"]),
               (b["rows"], b["a_s"], b["a_e"], b["ok"])]
        res = list(pipe.run(mbs))
    finally:
        pipe.close()
    assert len(res) == 3 and all(isinstance(r, pipeline.BoostMinibatch) for r in res)
    for r, want in zip(res, (en, e, e)):
        got = dict(vars(r.fingerprints), prob=r.prob, pred=r.pred.astype(np.int32), conf=r.conf)
        _check(got, want, "pipeline")
        assert r.pred.dtype == np.int64 and r.dist is None and (r.call == -1).all() and _same(r.status, want["status"])
        assert (r.fingerprints.refine_idx is not None) == refine


def test_feeder_with_a_boost_model_forked_workers():
    """Feeder(model=Fpt_Boost) from four forked workers -- refine and plain rings, float32 then int16 --, `predict`, and a ring
    whose n_classes is not the model's k, in a fresh interpreter whose parent never touches the GPU
    (tests/helpers/feeder_boost_check.py)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "feeder_boost_check.py")], capture_output=True,
                       text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["gpu_processes"] <= 6
    for run in ("refine float32", "refine int16", "plain float32", "plain int16", "predict"):
        assert rec[run] and all(rec[run].values()), (run, rec[run])
    assert rec["mismatch"] == {"first": "INVALID", "second": "INVALID", "predict": "INVALID", "still_serving": True}
    assert rec["refused"] == {"demux_without_references": True}


def test_feeder_refuses_an_svm_of_another_class_count():
    """The same mismatch on the SVM side: a ring laid out for 3 classes, a resident DTW_SVM with 4.  WDX_WANT_SVM through
    wdx_feeder_run and wdx_feeder_predict is answered WDX_ERR_INVALID naming both counts, minibatch by minibatch; the feeder
    keeps serving what needs no tail and ends with every slot free (tests/helpers/feeder_svm_mismatch_check.py)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "feeder_svm_mismatch_check.py")],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["model_classes"] == 4
    for call in ("run", "predict", "run_again"):
        assert "the SVM model has 4 classes" in rec[call] and "laid out for 3 and 25" in rec[call], (call, rec[call])
    assert rec["served_without_the_tail"] is True and rec["alive"] is True
    assert rec["stats"]["free_slots"] == rec["stats"]["n_slots"] == 2 and rec["stats"]["served"] == 5
