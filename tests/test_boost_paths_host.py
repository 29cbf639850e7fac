"""The Fpt_Boost tail through the host-fed paths (WDX_WANT_BOOST, wdx_feeder_predict_boost, MinibatchPipeline / Feeder with
``model=Fpt_Boost``): what can be checked without a GPU -- the constants against the header, the new export's signature,
the Python constructors' refusals and the argument checks of the feeder's worker calls, which run before a slot is claimed
(the no-GPU ring hooks, as tests/test_refine_paths_host.py uses them)."""
import ctypes as C
import mmap
import os
import re

import numpy as np
import pytest

from helpers import boost_ref
from warpdemux_amd import _lib, feeder, models, pipeline, sig_proc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 25
INV = _lib.WDX_ERR_INVALID


def _boost(n_features=K, dim=4):
    m = boost_ref.random_model(3, 2, dim, n_features, seed=1)
    trees = [(f, b, [False] * len(f), lv) for f, b, lv in m.trees]
    return models.Fpt_Boost(trees, m.n_features, m.scale, m.bias, {i: i for i in range(m.k)})


def _ring(n_classes, n_events=K, n_refs=0, refine=False, fmt=_lib.FEEDER_SAMPLES_FLOAT32):
    """an initialised ring in zeroed page-aligned memory: (mmap kept alive, address)"""
    L = _lib.load()
    g = _lib.FeederGeometryC(3, n_events, n_classes, fmt, 50, 4000, n_refs)
    pc = sig_proc.SegParams(barcode_num_events=K).to_c()
    if refine:
        rc = sig_proc.RefineParams(query=np.linspace(-1.0, 1.0, 84), barcode_keep_events=K).to_c()
        m = mmap.mmap(-1, int(L.wdx_feeder_ring_bytes_refine(C.byref(g))))
        a = C.addressof(C.c_char.from_buffer(m))
        assert L.wdx_feeder_ring_init_refine(a, len(m), C.byref(g), C.byref(pc), C.byref(rc)) == 0
    else:
        m = mmap.mmap(-1, int(L.wdx_feeder_ring_bytes(C.byref(g))))
        a = C.addressof(C.c_char.from_buffer(m))
        assert L.wdx_feeder_ring_init(a, len(m), C.byref(g), C.byref(pc)) == 0
    return m, a


def test_constants_mirror_the_header_and_the_export_is_bound():
    hdr = open(os.path.join(ROOT, "include", "wdx.h")).read()

    def define(name):
        return int(re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", hdr, flags=re.M).group(1), 0)

    assert _lib.WANT_BOOST == 0x40 == define("WDX_WANT_BOOST")
    assert _lib.OPT_BOOST_KERNEL == 19 == define("WDX_OPT_BOOST_KERNEL")
    assert _lib.BOOST_SMALL_READS == define("WDX_BOOST_SMALL_READS")
    assert _lib.BOOST_TREE_CHUNK == define("WDX_BOOST_TREE_CHUNK")
    assert _lib.BOOST_SMALL_MAX_READS == define("WDX_BOOST_SMALL_MAX_READS")
    # what the kernel's carve-up relies on: 16-bit leaf indices, one (read, class) lane each in a 256-thread workgroup
    assert _lib.BOOST_SMALL_READS * _lib.BOOST_MAX_DIM <= 256 and _lib.BOOST_MAX_DEPTH <= 16
    assert define("WDX_ABI_VERSION") == 4 == _lib.ABI_VERSION
    # no bit of WDX_WANT_* is used twice
    bits = [getattr(_lib, k) for k in dir(_lib) if k.startswith("WANT_")]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)
    L = _lib.load()
    assert "wdx_feeder_predict_boost" in _lib.EXPORTS
    f = L.wdx_feeder_predict_boost
    assert f.argtypes == L.wdx_feeder_predict.argtypes and f.restype is C.c_int


def test_python_constructors_refuse_before_anything_is_created():
    with pytest.raises(ValueError, match="boost model takes 25 features"):
        pipeline.MinibatchPipeline(None, params=sig_proc.SegParams(barcode_num_events=24), model=_boost())
    with pytest.raises(ValueError, match="boost model takes 25 features"):
        pipeline.MinibatchPipeline(None, model=_boost(), refine=sig_proc.RefineParams(query=np.zeros(8), barcode_keep_events=20))
    with pytest.raises(ValueError, match="boost model takes 25 features"):
        pipeline.MinibatchPipeline(np.zeros((3, 24)), model=_boost())
    with pytest.raises(ValueError, match="boost model takes 25 features"):
        feeder.Feeder(model=_boost(), params=sig_proc.SegParams(barcode_num_events=24))
    with pytest.raises(ValueError, match="boost model takes 25 features"):
        feeder.Feeder(model=_boost(), refine=sig_proc.RefineParams(query=np.zeros(8), barcode_keep_events=20))
    # unchanged: nothing to serve
    with pytest.raises(ValueError, match="refs or model is required"):
        feeder.Feeder(refine=None, refs=None)
    with pytest.raises(ValueError, match="refs is required"):
        pipeline.MinibatchPipeline(None)


def test_demux_batch_is_refused_on_a_boost_feeder_without_references():
    """the refusal is the first statement of `demux_batch[_adc]`: a Feeder's fields without its ring and process"""
    f = feeder.Feeder.__new__(feeder.Feeder)
    f.nY, f.boost, f._shm, f._proc = 0, True, None, None
    sig = np.zeros((2, 400), dtype=np.float32)
    with pytest.raises(ValueError, match="fingerprint-only behind its boost model"):
        f.demux_batch(sig, [0, 0], [400, 400])
    with pytest.raises(ValueError, match="fingerprint-only"):
        f.demux_batch_adc(sig.astype(np.int16), [400, 400], [0, 0], [1, 1], [0, 0], [400, 400])


def _job(want, prob=True, pred=True, conf=True, keep=None):
    sig = np.zeros((2, 400), dtype=np.float32)
    a_s, a_e = np.zeros(2, dtype=np.int32), np.full(2, 400, dtype=np.int32)
    o = dict(status=np.empty(2, np.int32), fpt=np.empty((2, K)), prob=np.empty((2, 4)), pred=np.empty(2, np.int32), conf=np.empty(2))
    keep.extend([sig, a_s, a_e, o])
    return _lib.FeederJobC(_lib.addr(sig), 2, 400, _lib.addr(a_s), _lib.addr(a_e), None, want, 0, _lib.addr(o["status"]), None,
                           None, _lib.addr(o["fpt"]), None, None, _lib.addr(o["prob"]) if prob else None,
                           _lib.addr(o["pred"]) if pred else None, _lib.addr(o["conf"]) if conf else None)


@pytest.mark.parametrize("refine", [False, True], ids=["plain-ring", "refine-ring"])
def test_feeder_run_refuses_want_boost_before_it_claims_a_slot(refine):
    L = _lib.load()
    keep = []
    W = _lib
    run = (lambda a, j: L.wdx_feeder_run_refine(a, C.byref(j), None, None)) if refine else (lambda a, j: L.wdx_feeder_run(a, C.byref(j)))
    m0, a0 = _ring(0, refine=refine)                       # laid out without room for prob / pred / conf
    assert run(a0, _job(W.WANT_FPT | W.WANT_BOOST, keep=keep)) == INV
    assert b"n_classes 0" in L.wdx_last_error()
    m1, a1 = _ring(4, n_events=0, refine=refine)           # ... without room for fingerprints: nothing for the model to read
    assert run(a1, _job(W.WANT_BOOST, keep=keep)) == INV
    m2, a2 = _ring(4, refine=refine)
    assert run(a2, _job(W.WANT_FPT | W.WANT_SVM | W.WANT_BOOST, keep=keep)) == INV
    assert b"WDX_WANT_SVM and WDX_WANT_BOOST" in L.wdx_last_error()
    for missing in ("prob", "pred", "conf"):
        assert run(a2, _job(W.WANT_FPT | W.WANT_BOOST, keep=keep, **{missing: False})) == INV, missing
        assert b"no destination" in L.wdx_last_error()
    assert run(a2, _job(0x80 | W.WANT_BOOST, keep=keep)) == INV          # an unknown bit stays refused
    # every refusal came before a slot was claimed: all three are free
    free = C.c_int32(-1)
    for a in (a0, a1, a2):
        assert L.wdx_feeder_stats(a, None, None, C.byref(free)) == 0 and free.value == 3
    # int16 job on this float32 ring: the format check comes first, as for every other bit
    adc = np.zeros((2, 400), dtype=np.int16)
    ja = _lib.FeederJobAdcC(_lib.addr(adc), 2, 400, None, None, None, None, None, None, W.WANT_BOOST, 0, *([None] * 9))
    assert L.wdx_feeder_run_adc(a2, C.byref(ja)) == INV


def test_feeder_predict_boost_refuses_a_ring_without_a_model():
    L = _lib.load()
    X, prob, pred, conf = np.zeros((2, K)), np.empty((2, 4)), np.empty(2, np.int32), np.empty(2)
    args = (_lib.ptr(X), 2, _lib.ptr(prob), _lib.ptr(pred), _lib.ptr(conf))
    for kw in (dict(n_classes=0), dict(n_classes=4, n_events=0)):
        m, a = _ring(**kw)
        assert L.wdx_feeder_predict_boost(a, *args) == INV
        assert b"feeder_predict_boost" in L.wdx_last_error() and b"without a model" in L.wdx_last_error()
    m, a = _ring(4)
    assert L.wdx_feeder_predict_boost(a, None, 2, *args[2:]) == INV
    assert L.wdx_feeder_predict_boost(a, *args[:2], None, *args[3:]) == INV
    assert L.wdx_feeder_predict_boost(a, _lib.ptr(X), 0, None, None, None) == 0       # no rows: nothing to serve
    assert L.wdx_feeder_predict_boost(None, *args) == INV                             # not a ring
    # a stopped ring answers a claim at once: the call does get as far as the ring
    assert L.wdx_feeder_stop(a) == 0
    assert L.wdx_feeder_predict_boost(a, *args) == _lib.WDX_ERR_NO_DEVICE
