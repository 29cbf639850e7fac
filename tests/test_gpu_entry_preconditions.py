"""What every entry point with a classifier tail or a refinement branch answers when it must refuse: the return code, and
that nothing the caller handed over for results was written.  One table; the codes are the ones the entry points returned
when each of them still spelt these checks out itself (tail_ready / refine_seg_params in warpdemux_amd/csrc state them once
now), so a code that shifts at one site fails here by name.

Argument refusals only: no case reaches a kernel, so the four reads are noise in rows of 2 048 samples (the stride of
tests/helpers/window_inputs.py) and the models hold one tree, one hidden layer and two support vectors.  Two contexts of
the module's own serve every case: `bare` holds references and no model, `odd` holds the same references and three models
that do not fit them -- an SVM trained on one reference more, an MLP with one input more, boosted trees over one feature
more than K."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from helpers import window_inputs as wi
from warpdemux_amd import _lib, sig_proc

pytestmark = pytest.mark.gpu

N, STRIDE, K, N_REFS = 4, wi.STRIDE, wi.K, wi.N_REFS
INV, NO_REFS = _lib.WDX_ERR_INVALID, _lib.WDX_ERR_NO_REFS
NONE, SVM, MLP, BOOST = _lib.LIVE_TAIL_NONE, _lib.LIVE_TAIL_SVM, _lib.LIVE_TAIL_MLP, _lib.LIVE_TAIL_BOOST
FILL = -9


def _seg(keep=K):
    return sig_proc.SegParams(**{**wi.SEG, "barcode_num_events": keep}).to_c()


def _refine(how=None):
    """the refinement parameters, or one way of getting them wrong"""
    rp = sig_proc.RefineParams(query=np.cos(0.3 * np.arange(40)), barcode_segm_events=K, barcode_keep_events=K)
    c = rp.to_c()
    c._keep = rp
    if how == "null query":
        c.query = None
    elif how == "empty query":
        c.n_query = 0
    elif how == "keep 0":
        c.barcode_keep_events = 0
    return c


class Env:
    """one context, its references [and the three models that do not fit], the minibatch on both sides of the bus and
    every result array an entry point can be handed, filled with FILL"""

    def __init__(self, models):
        self.L, self.ctx = _lib.load(), _lib.Context(0)
        rng = np.random.default_rng(5)
        refs = rng.normal(size=(N_REFS, K))
        _lib.check(self.L.wdx_set_refs(self.ctx.handle, _lib.ptr(refs), N_REFS, K, 5, 0.1))
        if models:
            self._set_models(rng)
        self.rows = rng.normal(size=(N, STRIDE)).astype(np.float32)
        self.a_s, self.a_e = np.full(N, 200, np.int32), np.full(N, 900, np.int32)
        self.ok, self.row_len = np.ones(N, np.uint8), np.full(N, STRIDE, np.int32)
        self.X = rng.normal(size=(N, K))
        self.d_in = {k: torch.from_numpy(getattr(self, k)).cuda() for k in ("rows", "a_s", "a_e", "ok")}
        kmax = 4
        shapes = dict(status=((N,), np.int32), call=((N,), np.int32), dist=((N, N_REFS + 1), np.float32), fpt=((N, K + 1), np.float64),
                      dwell=((N, K + 1), np.int64), stats=((N, 6), np.float64), refine_idx=((N, 3), np.int32),
                      raw=((N, kmax), np.float64), prob=((N, kmax), np.float64), pred=((N,), np.int32), conf=((N,), np.float64),
                      counts=((N_REFS + 1,), np.int64), bad=((1,), np.int64))
        self.host = {k: np.full(s, FILL, t) for k, (s, t) in shapes.items()}
        self.dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in self.host.items()}
        self.work = torch.empty(int(self.L.wdx_demux_refine_workspace_bytes(N, K + 1)), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def _set_models(self, rng):
        h, L = self.ctx.handle, self.L
        i32, f64 = (lambda *v: np.array(v, np.int32)), (lambda *v: np.array(v, np.float64))
        a = [i32(1, 1), i32(0, 1), f64(0.5, -0.5), f64(0.0), f64(-1.0), f64(0.0)]
        svm = _lib.SvmModelC(2, 2, N_REFS + 1, 1, 1.0, *[_lib.addr(v) for v in a], None, None)
        _lib.check(L.wdx_svm_set_model(h, C.byref(svm)))
        w = [rng.normal(size=(N_REFS + 1, 4)), rng.normal(size=(4, 2))]
        b = [np.zeros(4), np.zeros(2)]
        mlp = _lib.MlpModelC(n_layers=2, dtype_bytes=8, hidden_activation=_lib.MLP_ACT["relu"], n_classes=2, n_scalers=0)
        for i, v in enumerate((N_REFS + 1, 4, 2)):
            mlp.sizes[i] = v
        for i in range(2):
            mlp.coefs[i], mlp.intercepts[i] = _lib.addr(w[i]), _lib.addr(b[i])
        _lib.check(L.wdx_mlp_set_model(h, C.byref(mlp)))
        t = [i32(1), i32(0), np.zeros(1, np.float32), f64(0.0, 1.0, 1.0, 0.0), f64(0.0, 0.0)]
        boost = _lib.BoostModelC(1, K + 1, 2, 2, _lib.addr(t[0]), _lib.addr(t[1]), _lib.addr(t[2]), None, _lib.addr(t[3]), 1.0,
                                 _lib.addr(t[4]), None, None)
        _lib.check(L.wdx_boost_set_model(h, C.byref(boost)))

    # ---- the entry points: (self, p, rp, tail) -> code ------------------------------------------------------------------
    def _dev_reads(self):
        d = self.d_in
        return (self.ctx.handle, d["rows"].data_ptr(), None, None, STRIDE, STRIDE, N, d["a_s"].data_ptr(), d["a_e"].data_ptr(),
                d["ok"].data_ptr())

    def _d(self, *names):
        return [self.dev[k].data_ptr() for k in names]

    def demux_svm_dev(self, p, rp, tail):
        return self.L.wdx_demux_svm_dev(*self._dev_reads(), C.byref(p), *self._d("fpt", "status", "dist", "prob", "pred", "conf"),
                                        self.work.data_ptr(), 0, None)

    def demux_mlp_dev(self, p, rp, tail):
        return self.L.wdx_demux_mlp_dev(*self._dev_reads(), C.byref(p), *self._d("fpt", "status", "dist", "prob", "pred", "conf", "bad"),
                                        self.work.data_ptr(), 0, None)

    def demux_boost_dev(self, p, rp, tail):
        return self.L.wdx_demux_boost_dev(*self._dev_reads(), C.byref(p), C.byref(rp) if rp else None,
                                          *self._d("fpt", "refine_idx", "status", "raw", "prob", "pred", "conf"), self.work.data_ptr(), None)

    def fingerprint_refine_dev(self, p, rp, tail):
        return self.L.wdx_fingerprint_refine_dev(*self._dev_reads(), C.byref(p), C.byref(rp),
                                                 *self._d("fpt", "dwell", "stats", "refine_idx", "status"), None)

    def demux_refine_dev(self, p, rp, tail):
        return self.L.wdx_demux_refine_dev(*self._dev_reads(), C.byref(p), C.byref(rp),
                                           *self._d("fpt", "dwell", "stats", "refine_idx", "status", "dist", "call", "counts"),
                                           self.work.data_ptr(), None)

    def fingerprint_refine_batch(self, p, rp, tail):
        o = self.host
        return self.L.wdx_fingerprint_refine_batch(self.ctx.handle, _lib.ptr(self.rows), N, STRIDE, _lib.ptr(self.a_s), _lib.ptr(self.a_e),
                                                   _lib.ptr(self.ok), C.byref(p), C.byref(rp), _lib.ptr(o["fpt"]), _lib.ptr(o["dwell"]),
                                                   _lib.ptr(o["stats"]), _lib.ptr(o["refine_idx"]), _lib.ptr(o["status"]))

    def dtw_svm_predict(self, p, rp, tail):
        o = self.host
        return self.L.wdx_dtw_svm_predict(self.ctx.handle, _lib.ptr(self.X), N, _lib.ptr(o["prob"]), _lib.ptr(o["pred"]), _lib.ptr(o["conf"]))

    def dtw_mlp_predict(self, p, rp, tail):
        o = self.host
        return self.L.wdx_dtw_mlp_predict(self.ctx.handle, _lib.ptr(self.X), N, _lib.ptr(o["prob"]), _lib.ptr(o["pred"]), _lib.ptr(o["conf"]),
                                          o["bad"].ctypes.data_as(C.POINTER(C.c_int64)))

    def _minibatch(self):
        return _lib.MinibatchInC(_lib.addr(self.rows), N, STRIDE, None, None, _lib.addr(self.a_s), _lib.addr(self.a_e), _lib.addr(self.ok))

    def _nothing_in_the_slot(self):
        """a refused submit leaves the slot free: the wait finds nothing (and writes nothing)"""
        self.msg = self.L.wdx_last_error()    # (the submit's: the wait below leaves its own)
        o = self.host
        out = _lib.MinibatchOutC(*[_lib.addr(o[k]) for k in ("status", "call", "dist", "fpt", "dwell", "stats", "prob", "pred", "conf")])
        assert self.L.wdx_demux_wait_refine(self.ctx.handle, 0, C.byref(out), _lib.ptr(o["refine_idx"])) == INV

    def demux_submit_ex(self, p, rp, tail):
        mb = self._minibatch()
        code = self.L.wdx_demux_submit_ex(self.ctx.handle, 0, C.byref(mb), C.byref(p), N_REFS,
                                          _lib.WANT_FPT | {SVM: _lib.WANT_SVM, BOOST: _lib.WANT_BOOST}[tail])
        self._nothing_in_the_slot()
        return code

    def demux_submit_refine(self, p, rp, tail):
        mb = self._minibatch()
        code = self.L.wdx_demux_submit_refine(self.ctx.handle, 0, C.byref(mb), None, C.byref(p), C.byref(rp), N_REFS,
                                              _lib.WANT_FPT | _lib.WANT_REFINE_IDX | (_lib.WANT_BOOST if tail == BOOST else 0))
        self._nothing_in_the_slot()
        return code

    def live_tick_ex(self, p, rp, tail):
        o = self.host
        ptrs = (C.c_void_p * N)(*[self.rows[i].ctypes.data for i in range(N)])
        desc = _lib.LiveInC(C.cast(ptrs, C.c_void_p), None, None, None, _lib.addr(self.row_len), N, _lib.addr(self.a_s), _lib.addr(self.a_e),
                            _lib.addr(self.ok), tail, 0)
        out = _lib.MinibatchOutC(*[_lib.addr(o[k]) for k in ("status", "call", "dist", "fpt", "dwell", "stats", "prob", "pred", "conf")])
        want = _lib.WANT_FPT | (_lib.WANT_REFINE_IDX if rp else 0)
        return self.L.wdx_live_tick_ex(self.ctx.handle, C.byref(desc), C.byref(p), C.byref(rp) if rp else None, N_REFS, want, C.byref(out),
                                       _lib.ptr(o["refine_idx"]), o["bad"].ctypes.data_as(C.POINTER(C.c_int64)))

    def refused(self, entry, p, rp, tail):
        """code and message of one call"""
        self.msg = None
        code = getattr(self, entry)(p, rp, tail)
        return code, self.msg or self.L.wdx_last_error()

    def touched(self):
        torch.cuda.synchronize()
        return [k for k, v in self.host.items() if (v != FILL).any()] + [k for k, v in self.dev.items() if bool((v != FILL).any())]


@functools.lru_cache(maxsize=None)
def _env(models):
    return Env(models)


PLAIN_WORDS = b"barcode_num_events (%d) != the boost model's features (%d)" % (K, K + 1)
REFINED_WORDS = b"barcode_keep_events (%d) != the boost model's features (%d)" % (K, K + 1)
DTW_TAIL_ENTRIES = [("demux_svm_dev", SVM), ("demux_mlp_dev", MLP), ("dtw_svm_predict", SVM), ("dtw_mlp_predict", MLP),
                    ("demux_submit_ex", SVM), ("live_tick_ex", MLP)]
REFINE_ENTRIES = ["demux_boost_dev", "demux_submit_refine", "live_tick_ex", "fingerprint_refine_dev", "fingerprint_refine_batch",
                  "demux_refine_dev"]
# (entry point, tail, refusal, context, refinement parameters, code, words of the message or None)
TABLE = (
    # no model: every tail of every entry point that takes one
    [(e, t, "no model", False, None, NO_REFS, None) for e, t in DTW_TAIL_ENTRIES + [("live_tick_ex", SVM)]]
    + [(e, BOOST, "no model", False, None, NO_REFS, None) for e in ("demux_boost_dev", "demux_submit_ex", "live_tick_ex")]
    + [(e, BOOST, "no model, refined", False, "ok", NO_REFS, None) for e in ("demux_boost_dev", "demux_submit_refine", "live_tick_ex")]
    # a model that was trained on another reference set
    + [(e, t, "model/reference mismatch", True, None, INV, None) for e, t in DTW_TAIL_ENTRIES]
    # (the live tick answers an SVM of another set as it answers no SVM; every other entry point tells the two apart)
    + [("live_tick_ex", SVM, "model/reference mismatch", True, None, NO_REFS, None)]
    # boosted trees over another number of features, K named as the caller set it
    + [(e, BOOST, "feature count", True, None, INV, PLAIN_WORDS) for e in ("demux_boost_dev", "demux_submit_ex", "live_tick_ex")]
    + [(e, BOOST, "feature count, refined", True, "ok", INV, REFINED_WORDS)
       for e in ("demux_boost_dev", "demux_submit_refine", "live_tick_ex")]
    # the refinement parameters
    + [(e, NONE, how, False, how, INV, None) for how in ("null query", "empty query") for e in REFINE_ENTRIES]
    + [(e, NONE, "keep 0", False, "keep 0", INV, None) for e in ("demux_submit_refine", "live_tick_ex", "fingerprint_refine_batch")]
)
TAIL_NAMES = {NONE: "none", SVM: "svm", MLP: "mlp", BOOST: "boost"}


@pytest.mark.parametrize("entry,tail,refusal,models,refine,code,words", TABLE,
                         ids=[f"{e}-{TAIL_NAMES[t]}-{r.replace(' ', '_')}" for e, t, r, *_ in TABLE])
def test_refusal_returns_its_code_and_writes_nothing(entry, tail, refusal, models, refine, code, words):
    env = _env(models)
    rp = None if refine is None else _refine(None if refine == "ok" else refine)
    got, msg = env.refused(entry, _seg(), rp, tail)
    assert got == code, (got, msg)
    assert words is None or words in msg, msg
    assert env.touched() == [], "a refused call wrote an output"


def test_the_table_names_every_entry_point_and_refusal():
    assert {e for e, *_ in TABLE} == {"demux_svm_dev", "demux_mlp_dev", "demux_boost_dev", "dtw_svm_predict", "dtw_mlp_predict",
                                      "demux_submit_ex", "demux_submit_refine", "live_tick_ex", "fingerprint_refine_dev",
                                      "fingerprint_refine_batch", "demux_refine_dev"}
    assert {r.split(",")[0] for _, _, r, *_ in TABLE} == {"no model", "model/reference mismatch", "feature count", "null query",
                                                          "empty query", "keep 0"}
