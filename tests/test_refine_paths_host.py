"""Consensus refinement through the minibatch, feeder and fused entry points: what can be checked without a GPU -- the
new symbols and their ctypes signatures, the feeder ring's two layouts, the argument checks that run before any device
call, and the ReadResult helper the blocking shim and the feeder's workers share."""
import ctypes as C
import mmap
from types import SimpleNamespace as NS

import numpy as np
import pytest

from warpdemux_amd import _lib, feeder, pipeline, sig_proc

NEW = ("wdx_demux_submit_refine", "wdx_demux_wait_refine", "wdx_demux_refine_workspace_bytes", "wdx_demux_refine_dev",
       "wdx_feeder_ring_bytes_refine", "wdx_feeder_ring_init_refine", "wdx_feeder_run_refine")


def _geo(n_refs=4, n_events=25, fmt=_lib.FEEDER_SAMPLES_FLOAT32):
    return _lib.FeederGeometryC(3, n_events, 0, fmt, 50, 4000, n_refs)


def _ring(nbytes):
    """zeroed page-aligned memory and its address"""
    m = mmap.mmap(-1, nbytes)
    return m, C.addressof(C.c_char.from_buffer(m))


def _refine(n_query=84, **kw):
    return sig_proc.RefineParams(query=np.linspace(-1.0, 1.0, max(n_query, 1)), **kw)


def test_new_symbols_and_signatures():
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS
        f = getattr(L, name)
        assert f.argtypes is not None and f.restype is not None, name
    assert _lib.WANT_REFINE_IDX == 0x20
    assert L.wdx_demux_refine_workspace_bytes(0, 0) == 0
    for n in (1, 96, 8192):   # the plain call's pieces, rounded to 256, plus one 1632-byte hand-over record per read
        base = L.wdx_demux_workspace_bytes(n, 25)
        assert L.wdx_demux_refine_workspace_bytes(n, 25) == (base + 255) // 256 * 256 + 1632 * n


def test_plain_ring_keeps_its_bytes():
    """a ring made by wdx_feeder_ring_init: the same bytes before and after the refine code path ran in this process"""
    L = _lib.load()
    pc = sig_proc.SegParams(barcode_num_events=25).to_c()
    images = []
    for touch in (False, True):
        if touch:
            g2, rc = _geo(n_refs=0), _refine().to_c()
            m2, a2 = _ring(int(L.wdx_feeder_ring_bytes_refine(C.byref(g2))))
            assert L.wdx_feeder_ring_init_refine(a2, len(m2), C.byref(g2), C.byref(pc), C.byref(rc)) == 0
        g = _geo()
        nbytes = int(L.wdx_feeder_ring_bytes(C.byref(g)))
        m, a = _ring(nbytes)
        assert L.wdx_feeder_ring_init(a, nbytes, C.byref(g), C.byref(pc)) == 0
        images.append(bytes(m[:]))
    assert images[0] == images[1]
    assert not np.frombuffer(images[0], dtype=np.uint8)[4096 * 3:].any(), "the data regions of a fresh ring are untouched"


def test_refine_ring_limits_and_geometry():
    L = _lib.load()
    g = _geo()
    plain, refine = int(L.wdx_feeder_ring_bytes(C.byref(g))), int(L.wdx_feeder_ring_bytes_refine(C.byref(g)))
    assert refine == plain + 3 * 4096, "one refine_idx region (50 x 12 bytes -> one page) per slot, the header as large"
    m, a = _ring(refine)
    ok = sig_proc.SegParams(num_events=120, barcode_num_events=7)   # (barcode_num_events is ignored: K = keep)

    def init(geo, params, rp):
        pc, rc = params.to_c(), rp.to_c()
        return L.wdx_feeder_ring_init_refine(a, refine, C.byref(geo), C.byref(pc), C.byref(rc))

    assert init(g, ok, _refine()) == _lib.WDX_SUCCESS
    assert init(g, ok, _refine(96)) == _lib.WDX_SUCCESS
    rc0 = _refine(1).to_c()
    rc0.n_query = 0
    pc = ok.to_c()
    assert L.wdx_feeder_ring_init_refine(a, refine, C.byref(g), C.byref(pc), C.byref(rc0)) == _lib.WDX_ERR_INVALID
    assert init(g, ok, _refine(97)) == _lib.WDX_ERR_UNSUPPORTED          # the blocking call's code for this limit
    assert init(g, sig_proc.SegParams(num_events=127), _refine()) == _lib.WDX_SUCCESS
    assert init(g, sig_proc.SegParams(num_events=128), _refine()) == _lib.WDX_ERR_UNSUPPORTED
    assert init(_geo(n_refs=0), ok, _refine()) == _lib.WDX_SUCCESS       # fingerprint-only ring
    assert init(_geo(n_events=24), ok, _refine()) == _lib.WDX_ERR_INVALID   # n_events must be rp.barcode_keep_events
    assert L.wdx_feeder_ring_init_refine(a, refine - 1, C.byref(g), C.byref(pc), C.byref(_refine().to_c())) == _lib.WDX_ERR_INVALID


def test_refine_idx_is_refused_on_a_plain_ring_and_fingerprint_only_rings_serve_no_distances():
    L = _lib.load()
    pc = sig_proc.SegParams(barcode_num_events=25).to_c()
    sig = np.zeros((2, 400), dtype=np.float32)
    a_s, a_e = np.zeros(2, dtype=np.int32), np.full(2, 400, dtype=np.int32)
    status, idx, dist = np.empty(2, np.int32), np.empty((2, 3), np.int32), np.empty((2, 4), np.float32)
    fpt = np.empty((2, 25))

    def job(want):
        return _lib.FeederJobC(_lib.addr(sig), 2, 400, _lib.addr(a_s), _lib.addr(a_e), None, want, 0, _lib.addr(status), None,
                               _lib.addr(dist), _lib.addr(fpt), None, None, None, None, None)

    g = _geo()
    m, a = _ring(int(L.wdx_feeder_ring_bytes(C.byref(g))))
    assert L.wdx_feeder_ring_init(a, len(m), C.byref(g), C.byref(pc)) == 0
    j = job(_lib.WANT_FPT | _lib.WANT_REFINE_IDX)
    assert L.wdx_feeder_run_refine(a, C.byref(j), None, _lib.ptr(idx)) == _lib.WDX_ERR_INVALID
    assert b"WDX_WANT_REFINE_IDX" in L.wdx_last_error()
    assert L.wdx_feeder_run_refine(a, None, None, _lib.ptr(idx)) == _lib.WDX_ERR_INVALID
    g0, rc = _geo(n_refs=0), _refine().to_c()
    m0, a0 = _ring(int(L.wdx_feeder_ring_bytes_refine(C.byref(g0))))
    assert L.wdx_feeder_ring_init_refine(a0, len(m0), C.byref(g0), C.byref(pc), C.byref(rc)) == 0
    j = job(_lib.WANT_FPT | _lib.WANT_DIST)
    assert L.wdx_feeder_run_refine(a0, C.byref(j), None, None) == _lib.WDX_ERR_INVALID
    j = job(_lib.WANT_FPT | _lib.WANT_REFINE_IDX)           # asked for, no destination
    assert L.wdx_feeder_run_refine(a0, C.byref(j), None, None) == _lib.WDX_ERR_INVALID


def test_python_front_doors_without_references():
    with pytest.raises(ValueError, match="refs or model is required"):
        feeder.Feeder(refine=None, refs=None)
    with pytest.raises(ValueError, match="refs or model is required"):
        feeder.Feeder()
    with pytest.raises(ValueError, match="refs is required"):
        pipeline.MinibatchPipeline(None)
    with pytest.raises(ValueError, match="reference length"):      # K = keep events must be the reference length
        feeder.Feeder(refs=np.zeros((3, 24)), refine=_refine(barcode_keep_events=25))
    with pytest.raises(NotImplementedError, match="refinement_optimal_cpts"):
        sig_proc.RefineParams.from_spc(NS(segmentation=NS(refinement_optimal_cpts=True)), np.zeros(4))


def test_read_results_helper_is_what_the_blocking_shim_returns(monkeypatch):
    """`read_results_from_batch(..., refined=True)` on a hand-made batch against `detect_results_to_fpt_batch` fed the
    same batch in place of the device call: one code path, the three refinement fields included"""
    n, K = 7, 5
    rng = np.random.default_rng(3)
    status = np.array([0, 6, 1, 3, 5, 0, 2], dtype=np.int32)
    fb = sig_proc.FingerprintBatch(rng.normal(size=(n, K)), rng.integers(5, 60, (n, K)).astype(np.int64),
                                   rng.normal(size=(n, 6)), status,
                                   np.where(np.isin(status, (0, 6))[:, None], rng.integers(0, 3000, (n, 3)), -1).astype(np.int32))
    drs = [sig_proc.DetectResults(st != 1, "" if st != 1 else "no adapter", 100 + i, 3000 + i) for i, st in enumerate(status)]
    ids = [f"read{i}" for i in range(n)]
    spc = NS(sig_extract=NS(padding=100, normalization="none"), core=NS(sig_norm_outlier_thresh=5.0),
             segmentation=NS(min_obs_per_base=9, running_stat_width=18, num_events=120, accept_less_cpts=False,
                             normalization="mean", barcode_num_events=[25, K], consensus_refinement=True,
                             consensus_subseq_match_normalization="mean", consensus_subseq_match_penalty=1.5,
                             consensus_subseq_match_psi=[5, 0, 40, 0], consensus_subseq_match_ub_start=18,
                             consensus_subseq_match_lb_end=69, consensus_subseq_match_ub_end=97,
                             refinement_optimal_cpts=False))
    seen = {}

    def fake(signals, a_s, a_e, params, refine, success=None, device=None):
        seen["K"], seen["ok"] = refine.barcode_keep_events, np.asarray(success).tolist()
        return fb

    monkeypatch.setattr(sig_proc, "fingerprint_refine_batch", fake)
    shim = sig_proc.detect_results_to_fpt_batch(np.zeros((n, 10), np.float32), spc, drs, ids, consensus_query=np.ones(8))
    mine = sig_proc.read_results_from_batch(fb, drs, ids, refined=True)
    assert seen == {"K": K, "ok": [int(s != 1) for s in status]}
    assert len(shim) == len(mine) == n
    for i, (x, y) in enumerate(zip(shim, mine)):
        dx, dy = dict(vars(x)), dict(vars(y))
        for key in ("barcode_fpt", "dwell_times"):
            vx, vy = dx.pop(key), dy.pop(key)
            assert (vx is None and vy is None) or np.array_equal(vx, vy), (i, key)
        assert dx == dy, i
        if status[i] in (0, 6):
            assert (y.seg_cons_query_start, y.seg_cons_query_end, y.sig_barcode_start) == tuple(int(v) for v in fb.refine_idx[i])
            assert y.success == (status[i] == 0)
        else:
            assert y.seg_cons_query_start is None and y.sig_barcode_start is None
    assert mine[1].fail_reason == "consensus query outlier" and mine[2].fail_reason == "no adapter"
