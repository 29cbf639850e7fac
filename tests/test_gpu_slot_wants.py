"""What a pipelined slot hands back follows what was asked for, and nothing else is written: wdx_demux_submit_ex / _adc /
_refine with every single WDX_WANT_* bit, all of them and none, against the run that asked for everything -- wanted arrays
bit for bit (NaN by position), every other array as it was (-9).  Three configurations, float32 and int16 rows, 37 reads:
    svm      references resident, the SVM tail
    boost    no references (n_refs = 0), the boost tail (whose bit such a minibatch cannot go without)
    refine   consensus refinement against resident references, WDX_WANT_REFINE_IDX among the bits
and two things around them: a wait refused for a refine_idx that does not match the submit writes nothing and can be
repeated with the right arguments, and an empty submit (n = 0) followed by its wait succeeds and writes nothing.
(The same two properties of a live tick: tests/test_gpu_live_ex.py.)"""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import boost_ref, refine_inputs as ri, svm_ref
from warpdemux_amd import _lib, models, sig_proc

pytestmark = pytest.mark.gpu

W = _lib
N, N_REFS, K, SEED = 37, 16, 25, 101
INV = _lib.WDX_ERR_INVALID
FP_BITS = (W.WANT_FPT, W.WANT_DWELL, W.WANT_STATS)
# name -> (refine, n_refs, bits always set, bits asked for one by one)
CONFIGS = {"svm": (False, N_REFS, 0, FP_BITS + (W.WANT_DIST, W.WANT_SVM)),
           "boost": (False, 0, W.WANT_BOOST, FP_BITS),
           "refine": (True, N_REFS, 0, FP_BITS + (W.WANT_DIST, W.WANT_REFINE_IDX))}
# the arrays of a wait and the bit that asks for each (status and call always come back)
ARRAYS = dict(status=0, call=0, dist=W.WANT_DIST, fpt=W.WANT_FPT, dwell=W.WANT_DWELL, stats=W.WANT_STATS,
              prob=W.WANT_SVM | W.WANT_BOOST, pred=W.WANT_SVM | W.WANT_BOOST, conf=W.WANT_SVM | W.WANT_BOOST,
              refine_idx=W.WANT_REFINE_IDX)


def _hp():
    return sig_proc.SegParams(barcode_num_events=K, **ri.SEG)


def _hr():
    return sig_proc.RefineParams(query=ri.consensus(), barcode_segm_events=25, barcode_keep_events=K)


@functools.lru_cache(maxsize=None)
def _batch():
    return ri.batch(SEED, N)


@functools.lru_cache(maxsize=None)
def _refs():
    b = _batch()
    fb = sig_proc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], _hp(), success=b["ok"])
    X = np.ascontiguousarray(fb.fpt[fb.status == 0][:N_REFS])
    assert X.shape == (N_REFS, K)
    return X


@functools.lru_cache(maxsize=None)
def _descriptor(fmt, n=N):
    """(descriptor, arrays kept alive) of the first n reads of the batch"""
    b = _batch()
    a_s, a_e, ok = (np.ascontiguousarray(b[key][:n]) for key in ("a_s", "a_e", "ok"))
    if fmt == "int16":
        v = sig_proc.adc_minibatch(np.ascontiguousarray(b["adc"][:n]), b["row_len"][:n].copy(), b["offset"][:n].copy(),
                                   b["scale"][:n].copy(), a_s, a_e, ok)
        return v[0], v[2]
    rows = np.ascontiguousarray(b["rows"][:n])
    ad = _lib.addr
    return _lib.MinibatchInC(ad(rows), n, rows.shape[1], None, None, ad(a_s), ad(a_e), ad(ok)), (rows, a_s, a_e, ok)


class Ctx:
    """one engine context with the references, an SVM trained on them and a boost model resident"""

    def __init__(self):
        self.L, self.ctx = _lib.load(), _lib.Context(0)
        _lib.check(self.L.wdx_set_refs(self.ctx.handle, _lib.ptr(_refs()), N_REFS, K, 15, 0.1))
        m = svm_ref.synth_model(3, seed=3, n_support=[4, 3, 5], n_extra=N_REFS - 12, thresholds=True, gamma=1e-3, pwr_dist=2)
        self.svm_model = m.to_dtw_svm(_refs())
        self.svm = self.svm_model.to_c()
        _lib.check(self.L.wdx_svm_set_model(self.ctx.handle, C.byref(self.svm)))
        bm = boost_ref.random_model(65, 6, 4, K, seed=81)
        trees = [(f, b, [False] * len(f), lv) for f, b, lv in bm.trees]
        self.boost_model = models.Fpt_Boost(trees, bm.n_features, bm.scale, bm.bias, {0: 7, 1: 1, 2: 10, 3: 4})
        self.boost = self.boost_model.to_c()
        _lib.check(self.L.wdx_boost_set_model(self.ctx.handle, C.byref(self.boost)))
        self.k = {"svm": 3, "boost": 4, "refine": 1}

    def submit(self, config, desc, want, slot=0):
        refine, n_refs, always, _bits = CONFIGS[config]
        pc, want = _hp().to_c(), want | always
        adc = isinstance(desc, _lib.MinibatchAdcInC)
        if refine:
            rc = _hr().to_c()
            return self.L.wdx_demux_submit_refine(self.ctx.handle, slot, None if adc else C.byref(desc),
                                                  C.byref(desc) if adc else None, C.byref(pc), C.byref(rc), n_refs, want)
        call = self.L.wdx_demux_submit_adc if adc else self.L.wdx_demux_submit_ex
        return call(self.ctx.handle, slot, C.byref(desc), C.byref(pc), n_refs, want)

    def arrays(self, config):
        """every destination a wait can name, filled with -9"""
        k = self.k[config]
        shapes = dict(status=((N,), np.int32), call=((N,), np.int32), dist=((N, N_REFS), np.float32), fpt=((N, K), np.float64),
                      dwell=((N, K), np.int64), stats=((N, 6), np.float64), prob=((N, k), np.float64), pred=((N,), np.int32),
                      conf=((N,), np.float64), refine_idx=((N, 3), np.int32))
        return {name: np.full(shape, -9, dtype) for name, (shape, dtype) in shapes.items()}

    def wait(self, o, given, slot=0):
        """wait with the arrays named in `given` (status and call always); the others are not shown to the library"""
        g = {name: (o[name] if name in given or name in ("status", "call") else None) for name in ARRAYS}
        out = _lib.MinibatchOutC(*[_lib.addr(g[key]) for key in ("status", "call", "dist", "fpt", "dwell", "stats", "prob", "pred", "conf")])
        return self.L.wdx_demux_wait_refine(self.ctx.handle, slot, C.byref(out), _lib.ptr(g["refine_idx"]))

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _untouched(a):
    return bool((a == -9).all())


def _wanted(config, want):
    want |= CONFIGS[config][2]
    return {name for name, bit in ARRAYS.items() if bit == 0 or (want & bit)}


_ALL = {}


def _all_wanted(c, config, fmt):
    """THE yardstick of a configuration: (mask, arrays) of the run that asks for every bit (computed once, never modified)"""
    if (config, fmt) not in _ALL:
        want = 0
        for bit in CONFIGS[config][3]:
            want |= bit
        o = c.arrays(config)
        assert c.submit(config, _descriptor(fmt)[0], want) == 0, c.L.wdx_last_error()
        assert c.wait(o, _wanted(config, want)) == 0, c.L.wdx_last_error()
        for name in _wanted(config, want):
            assert not _untouched(o[name]), name
            o[name].setflags(write=False)
        assert (o["status"] == 0).sum() >= 15 and o["status"][ri.I_DEAD] == 1
        assert (o["call"] == -1).all() if CONFIGS[config][1] == 0 else (o["call"][o["status"] == 0] >= 0).all()
        _ALL[config, fmt] = (want, o)
    return _ALL[config, fmt]


def _masks(config):
    bits = CONFIGS[config][3]
    every = 0
    for bit in bits:
        every |= bit
    return [0, every] + list(bits)


@pytest.mark.parametrize("fmt", ["float32", "int16"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_asking_for_less_returns_the_same_bits_and_writes_nothing_else(ctx, config, fmt):
    _, full = _all_wanted(ctx, config, fmt)
    for want in _masks(config):
        o = ctx.arrays(config)
        given = _wanted(config, want)
        if CONFIGS[config][1] == 0:
            given = given | {"dist"}            # (without references a `dist` array may be shown: it is left alone)
        assert ctx.submit(config, _descriptor(fmt)[0], want) == 0, ctx.L.wdx_last_error()
        assert ctx.wait(o, given) == 0, ctx.L.wdx_last_error()
        for name in ARRAYS:
            if name in _wanted(config, want):
                assert _same(o[name], full[name]), f"{config} {fmt} want {want:#x}: {name}"
            else:
                assert _untouched(o[name]), f"{config} {fmt} want {want:#x}: {name} was written"


@pytest.mark.parametrize("fmt", ["float32", "int16"])
def test_a_wait_refused_for_its_refine_idx_writes_nothing_and_can_be_repeated(ctx, fmt):
    every, full = _all_wanted(ctx, "refine", fmt)
    desc = _descriptor(fmt)[0]
    # refine_idx asked for, the wait does not take it
    o = ctx.arrays("refine")
    assert ctx.submit("refine", desc, every) == 0, ctx.L.wdx_last_error()
    assert ctx.wait(o, _wanted("refine", every) - {"refine_idx"}) == INV
    assert all(_untouched(a) for a in o.values()), "a refused wait wrote something"
    assert ctx.submit("refine", desc, every) == INV, "the slot still holds the minibatch"
    assert ctx.wait(o, _wanted("refine", every)) == 0, ctx.L.wdx_last_error()
    assert all(_same(o[name], full[name]) for name in ARRAYS)
    # refine_idx not asked for, the wait passes one
    want = every & ~W.WANT_REFINE_IDX
    o = ctx.arrays("refine")
    assert ctx.submit("refine", desc, want) == 0, ctx.L.wdx_last_error()
    assert ctx.wait(o, _wanted("refine", every)) == INV
    assert all(_untouched(a) for a in o.values()), "a refused wait wrote something"
    assert ctx.wait(o, _wanted("refine", want)) == 0, ctx.L.wdx_last_error()
    assert all(_same(o[name], full[name]) for name in _wanted("refine", want)) and _untouched(o["refine_idx"])


@pytest.mark.parametrize("fmt", ["float32", "int16"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_an_empty_submit_and_its_wait_succeed_and_write_nothing(ctx, config, fmt):
    _all_wanted(ctx, config, fmt)               # (the slot has served a full minibatch before: nothing of it comes back)
    want = _masks(config)[1]
    o = ctx.arrays(config)
    assert ctx.submit(config, _descriptor(fmt, 0)[0], want) == 0, ctx.L.wdx_last_error()
    assert ctx.wait(o, _wanted(config, want)) == 0, ctx.L.wdx_last_error()
    assert all(_untouched(a) for a in o.values())
    assert ctx.wait(o, _wanted(config, want)) == INV, "the slot is free again"
