"""wdx_live_tick_ex / LiveDemux.tick[_adc] / demux_worker for every model kind, both fingerprint branches and both sample
formats.  The yardstick is always a call that existed before the tick learnt any of this, on the same reads:
`sig_proc.fingerprint_batch[_adc]` / `fingerprint_refine_batch` (status, fpt, dwell, stats, refine_idx), `demux_batch[_adc]`
and `parallel_distances.nearest_reference` (call, dist), `wdx_dtw_svm_predict`, `wdx_dtw_mlp_predict`, `wdx_boost_predict`
(prob, pred, conf of the successful reads; a failed read carries pred -1 and NaN).  Every array bit for bit, NaN by position;
no tolerances.

Reads: tests/helpers/refine_inputs.py, the first n of one batch in an order fixed with the CPU oracle -- ragged rows of
2 500 .. 6 000 samples with a failed detection, a window far too short, consensus outliers and a window that runs past its
read's end among the first 17, and more successes than failures in every prefix the tests take.  The
two formats see that last read differently, by their contracts: a float32 tick's row ends with the read, so the window is
cut there (the yardstick for that read is the blocking call on a minibatch as wide as the read); an int16 row stands for
the calibrated samples and a NaN tail, so the window reads NaN as it does in an int16 minibatch."""
import ctypes as C
import functools
import queue
import threading

import numpy as np
import pytest

from helpers import boost_ref, mlp_ref, refine_inputs as ri
from oracle import wdx_oracle as orc
from warpdemux_amd import _lib, models, parallel_distances as pdist, sig_proc
from warpdemux_amd.live import LiveDemux, demux_worker

pytestmark = pytest.mark.gpu

SEED, N_REFS, K = 101, 16, 25
W = _lib
INV, NO_REFS = _lib.WDX_ERR_INVALID, _lib.WDX_ERR_NO_REFS
NONE, SVM, MLP, BOOST = _lib.LIVE_TAIL_NONE, _lib.LIVE_TAIL_SVM, _lib.LIVE_TAIL_MLP, _lib.LIVE_TAIL_BOOST
SIZES = (0, 1, 17, 65)     # 17: one past the MLP kernel's 16-row tile; 65: one past a wave of the lane-per-read kernels
THR = np.array([0.05, 0.2, 0.1, 0.3])
P_DEAD, P_SHORT, P_TAIL = 1, 2, 3      # where _batch puts the special reads of refine_inputs
NAMES = ("status", "call", "dist", "fpt", "dwell", "stats", "refine_idx", "prob", "pred", "conf")


def _hp(keep=K):
    return sig_proc.SegParams(barcode_num_events=keep, **ri.SEG)


def _hr(keep=K):
    return sig_proc.RefineParams(query=ri.consensus(), barcode_segm_events=25, barcode_keep_events=keep)


@functools.lru_cache(maxsize=None)
def _batch(variant="tick"):
    """refine_inputs' batch; "worker": every row cut to start at its window, adapter_start 0 and no success flags, which is
    what a live session queues (worker.py:39-44) -- the same windows, so the same fingerprints"""
    b = dict(ri.batch(SEED))
    # The order of the reads, chosen with the CPU oracle so that every prefix the tests take holds at least as many
    # successes as failures in BOTH branches: a success first, then the failed detection, the short window, the window
    # past its read's end and two consensus outliers, then the reads that succeed in both branches, then the rest.
    op = orc.SegParams(barcode_num_events=K, clip_bounds_f64=bool(_hp().to_c().clip_bounds_f64), **ri.SEG)
    o_ref = orc.fingerprint_refine_batch(b["rows"], b["a_s"], b["a_e"], op, orc.RefineParams(query=ri.consensus()), ok=b["ok"])[4]
    o_pln = orc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], op, ok=b["ok"])[3]
    both = [i for i in np.flatnonzero((o_ref == 0) & (o_pln == 0)) if i not in (ri.I_DEAD, ri.I_SHORT, ri.I_TAIL)]
    out6 = [i for i in np.flatnonzero(o_ref == 6) if i != ri.I_TAIL][:2]
    head = [both[0], ri.I_DEAD, ri.I_SHORT, ri.I_TAIL, *out6]
    order = head + both[1:]
    order += [i for i in range(len(o_ref)) if i not in order]
    assert len(both) >= 40 and len(out6) == 2 and sorted(order) == list(range(len(o_ref)))
    for key, v in b.items():
        if isinstance(v, np.ndarray):
            b[key] = np.ascontiguousarray(v[order])
    if variant == "worker":
        n, stride = b["rows"].shape
        st = np.maximum(b["a_s"].astype(np.int64) - b["padding"], 0)
        rows, adc = np.full_like(b["rows"], np.nan), np.full_like(b["adc"], 12345)
        for i in range(n):
            rows[i, : stride - st[i]], adc[i, : stride - st[i]] = b["rows"][i, st[i]:], b["adc"][i, st[i]:]
        b.update(rows=rows, adc=adc, row_len=(b["row_len"] - st).astype(np.int32), a_s=np.zeros(n, np.int32),
                 a_e=(b["a_e"] - st).astype(np.int32), ok=np.ones(n, np.uint8))
    rl = b["row_len"][:17]
    assert (rl % 2 == 1).any() and (rl % 8 != 0).sum() >= 8, "odd row lengths and lengths off the int16 packing's 8-sample groups"
    assert int(b["a_e"][P_TAIL]) + b["padding"] > rl[P_TAIL]
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ---- models -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _plain_refs():
    b = _batch()
    fb = sig_proc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], _hp(), success=b["ok"])
    X = np.ascontiguousarray(fb.fpt[fb.status == 0][:N_REFS])
    assert X.shape == (N_REFS, K)
    return X


@functools.lru_cache(maxsize=None)
def _refine_refs():
    b = _batch()
    fb = sig_proc.fingerprint_refine_batch(b["rows"], b["a_s"], b["a_e"], _hp(), _hr(), success=b["ok"])
    return np.ascontiguousarray(fb.fpt[fb.status == 0][:N_REFS])


@functools.lru_cache(maxsize=None)
def _svm_model(k=4, n_train=48):
    """as tests/test_gpu_live.py builds its small model: an SVC on the DTW kernel of noisy copies of the references"""
    from sklearn.svm import SVC

    rng = np.random.default_rng(3)
    centers = _plain_refs()[:k]
    y = np.arange(n_train) % k
    Xtr = centers[y] + 0.3 * rng.normal(size=(n_train, K))
    Ktr = np.exp(-orc.dtw_matrix(Xtr, Xtr, 15, 0.1).astype(np.float64))
    svc = SVC(kernel="precomputed", probability=True, random_state=0).fit(Ktr, y)
    sp = orc.svm_params(svc)
    return models.DTW_SVM(Xtr, *sp[:6], {i: i + 1 for i in range(k)}, np.full(k, 0.2), 15, 0.1, block_size=500)


@functools.lru_cache(maxsize=None)
def _mlp_model(bad_ref=False):
    """as tests/test_gpu_mlp.py wraps its estimators; bad_ref: one reference holds an infinity, so every distance row does"""
    refs = _plain_refs().copy()
    if bad_ref:
        refs[3, 7] = np.inf
    est = mlp_ref.random_mlp(N_REFS, (17,), 5, np.float32, "relu", seed=21)
    ref = mlp_ref.DTW_MLP(est, refs, {i: 3 * i + 1 for i in range(5)}, np.full(5, 0.15), window=15, penalty=0.1, block_size=500)
    return models.from_reference(ref)


@functools.lru_cache(maxsize=None)
def _boost_model(n_features=K):
    m = boost_ref.random_model(65, 6, 4, n_features, seed=81)
    trees = [(f, b, [False] * len(f), lv) for f, b, lv in m.trees]
    return models.Fpt_Boost(trees, m.n_features, m.scale, m.bias, {0: 7, 1: 1, 2: 10, 3: 4}, THR)


def _predict(tail, model, X):
    """prob, pred int32, conf of the blocking predict call of the model's kind on fingerprints X"""
    n = len(X)
    k = model.n_classes if tail == SVM else model.k
    prob, pred, conf = np.empty((n, k)), np.empty(n, np.int32), np.empty(n)
    X = np.ascontiguousarray(X)
    L = _lib.load()
    ctx = model._ensure_resident()
    if tail == SVM:
        _lib.check(L.wdx_dtw_svm_predict(ctx.handle, _lib.ptr(X), n, _lib.ptr(prob), _lib.ptr(pred), _lib.ptr(conf)))
    elif tail == MLP:
        bad = C.c_int64(-1)
        _lib.check(L.wdx_dtw_mlp_predict(ctx.handle, _lib.ptr(X), n, _lib.ptr(prob), _lib.ptr(pred), _lib.ptr(conf), C.byref(bad)))
        assert bad.value == 0
    else:
        _lib.check(L.wdx_boost_predict(ctx.handle, _lib.ptr(X), n, None, _lib.ptr(prob), _lib.ptr(pred), _lib.ptr(conf)))
    return prob, pred, conf


# ---- the yardstick ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fingerprints(fmt, refine, n, variant="tick"):
    """the blocking fingerprint call on the first n reads as a minibatch (computed once, read-only)"""
    b = _batch(variant)
    a_s, a_e, ok, rl = b["a_s"][:n], b["a_e"][:n], b["ok"][:n], b["row_len"][:n]

    def run(sl, width):
        rows = np.ascontiguousarray(b["rows"][sl, :width])
        if refine:    # (the refinement branch has one blocking call: float32 rows, which ARE the int16 rows' calibration)
            fb = sig_proc.fingerprint_refine_batch(rows, a_s[sl], a_e[sl], _hp(), _hr(), success=ok[sl])
        elif fmt == "f32":
            fb = sig_proc.fingerprint_batch(rows, a_s[sl], a_e[sl], _hp(), success=ok[sl])
        else:
            fb = sig_proc.fingerprint_batch_adc(np.ascontiguousarray(b["adc"][sl, :width]), rl[sl], b["offset"][sl], b["scale"][sl],
                                                a_s[sl], a_e[sl], _hp(), success=ok[sl])
        return dict(status=fb.status, fpt=fb.fpt, dwell=fb.dwell, stats=fb.stats,
                    refine_idx=fb.refine_idx if refine else np.full((fb.status.size, 3), -1, np.int32))

    stride = b["rows"].shape[1]
    assert (a_e.astype(np.int64) + b["padding"] <= stride).all()     # the minibatch holds every window whole
    e = run(slice(0, n), stride)
    if fmt == "f32":   # a float32 tick's row ends with the read: the window is cut there, as in a minibatch of that width
        past = np.flatnonzero((a_e.astype(np.int64) + b["padding"] > rl) & (ok != 0))
        assert n < 17 or P_TAIL in past
        for i in past:
            one = run(slice(i, i + 1), int(rl[i]))
            for name in e:
                e[name][i] = one[name][0]
    # the CPU oracle on the same minibatch: at least half of the reads succeed, and the device agrees which
    op = orc.SegParams(barcode_num_events=K, clip_bounds_f64=bool(_hp().to_c().clip_bounds_f64), **ri.SEG)
    rows = b["rows"][:n]
    o_status = (orc.fingerprint_refine_batch(rows, a_s, a_e, op, orc.RefineParams(query=ri.consensus()), ok=ok)[4] if refine
                else orc.fingerprint_batch(rows, a_s, a_e, op, ok=ok)[3]) if n else np.zeros(0, np.int32)
    assert 2 * int((o_status == 0).sum()) >= n and 2 * int((e["status"] == 0).sum()) >= n, (o_status, e["status"])
    if fmt == "i16" or n < 17:
        assert np.array_equal(o_status, e["status"])
    if n >= 17 and variant == "tick":
        st = e["status"]
        assert st[P_DEAD] == 1 and st[P_SHORT] == 3 and (not refine or (st == 6).sum() >= 2), st
        assert fmt == "f32" or st[P_TAIL] != 0      # int16: the window reads the NaN tail
    for a in e.values():
        a.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def _yard(fmt, refine, tail, refs_kind, n, variant="tick"):
    """everything a tick returns, from blocking calls: refs_kind None | "plain" | "refine" | "svm" | "mlp" names the
    resident reference set"""
    e = dict(_fingerprints(fmt, refine, n, variant))
    ok = e["status"] == 0
    model = {SVM: _svm_model, MLP: _mlp_model, BOOST: _boost_model}.get(tail, lambda: None)()
    refs = {None: None, "plain": _plain_refs, "refine": _refine_refs, "svm": lambda: _svm_model()._X,
            "mlp": lambda: _mlp_model()._X}[refs_kind]
    e["call"] = np.full(n, -1, np.int32)
    e["dist"] = None
    if refs is not None:
        refs = refs()
        e["dist"] = np.full((n, len(refs)), np.nan, np.float32)
        if ok.any():
            D, am = pdist.nearest_reference(e["fpt"][ok], refs, 15, 0.1)
            e["dist"][ok], e["call"][ok] = D, am
        if not refine and n:   # ... and the blocking demux call, where there is one, says the same on the whole minibatch
            b = _batch(variant)
            sig_proc.set_references(refs, 15, 0.1)
            if fmt == "f32":
                db = sig_proc.demux_batch(b["rows"][:n], b["a_s"][:n], b["a_e"][:n], _hp(), success=b["ok"][:n], want_dist=True)
            else:
                db = sig_proc.demux_batch_adc(np.ascontiguousarray(b["adc"][:n]), b["row_len"][:n], b["offset"][:n], b["scale"][:n],
                                              b["a_s"][:n], b["a_e"][:n], _hp(), success=b["ok"][:n], want_dist=True)
            both = ok & (db.status == 0)     # (float32: all but the read whose window the tick cuts at the read's end)
            assert both.sum() >= ok.sum() - 1 and _same(db.dist[both], e["dist"][both]) and _same(db.call[both], e["call"][both])
    if model is not None:
        k = model.n_classes if tail == SVM else model.k
        e["prob"], e["pred"], e["conf"] = np.full((n, k), np.nan), np.full(n, -1, np.int32), np.full(n, np.nan)
        if ok.any():
            e["prob"][ok], e["pred"][ok], e["conf"][ok] = _predict(tail, model, e["fpt"][ok])
            assert n < 17 or len(set(e["pred"][ok].tolist())) >= 2
    for a in e.values():
        if a is not None:
            a.setflags(write=False)
    return e


# ---- the tick through the C ABI ---------------------------------------------------------------------------------------

class Tick:
    """one engine context [+ references] [+ models], and wdx_live_tick_ex on the first n reads of the batch"""

    def __init__(self, refs=None, svm=None, mlp=None, boost=None):
        self.L, self.ctx = _lib.load(), _lib.Context(0)
        self.nY = 0 if refs is None else len(refs)
        if refs is not None:
            _lib.check(self.L.wdx_set_refs(self.ctx.handle, _lib.ptr(np.ascontiguousarray(refs)), self.nY, refs.shape[1], 15, 0.1))
        for m, setter in ((svm, self.L.wdx_svm_set_model), (mlp, self.L.wdx_mlp_set_model), (boost, self.L.wdx_boost_set_model)):
            if m is not None:
                mc = m.to_c()
                _lib.check(setter(self.ctx.handle, C.byref(mc)))

    def inputs(self, fmt, n, variant="tick"):
        b = _batch(variant)
        src = b["rows"] if fmt == "f32" else b["adc"]
        rows = [np.ascontiguousarray(src[i, : b["row_len"][i]]) for i in range(n)]
        ptrs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in rows])
        cut = lambda a: np.ascontiguousarray(a[:n])   # noqa: E731
        return dict(rows=rows, ptrs=ptrs, row_len=cut(b["row_len"]), a_s=cut(b["a_s"]), a_e=cut(b["a_e"]), ok=cut(b["ok"]),
                    offset=cut(b["offset"]), scale=cut(b["scale"]))

    def run(self, fmt, n, tail, refine, want, k=0, n_refs=None, keep=K, both_rows=False, no_rows=False, variant="tick", room=0):
        """room: the caller's arrays hold at least this many reads (an empty tick over non-empty arrays)"""
        n_reads, n = n, max(n, room)
        i = self.inputs(fmt, n, variant)
        p = C.cast(i["ptrs"], C.c_void_p)
        f32 = (fmt == "f32" or both_rows) and not no_rows
        i16 = (fmt == "i16" or both_rows) and not no_rows
        desc = _lib.LiveInC(p if f32 else None, p if i16 else None, _lib.addr(i["offset"]), _lib.addr(i["scale"]),
                            _lib.addr(i["row_len"]), n_reads, _lib.addr(i["a_s"]), _lib.addr(i["a_e"]), _lib.addr(i["ok"]), tail, 0)
        nY = self.nY if n_refs is None else n_refs
        o = dict(status=np.full(n, -9, np.int32), call=np.full(n, -9, np.int32), dist=np.full((n, max(nY, 1)), -9, np.float32),
                 fpt=np.full((n, keep), -9.0), dwell=np.full((n, keep), -9, np.int64), stats=np.full((n, 6), -9.0),
                 prob=np.full((n, max(k, 1)), -9.0), pred=np.full(n, -9, np.int32), conf=np.full(n, -9.0),
                 refine_idx=np.full((n, 3), -9, np.int32))
        out = _lib.MinibatchOutC(*[_lib.addr(o[key]) for key in ("status", "call", "dist", "fpt", "dwell", "stats", "prob", "pred", "conf")])
        pc, rc = _hp(keep).to_c(), _hr(keep).to_c()
        bad = C.c_int64(-1)
        code = self.L.wdx_live_tick_ex(self.ctx.handle, C.byref(desc), C.byref(pc), C.byref(rc) if refine else None, nY, want,
                                       C.byref(out), _lib.ptr(o["refine_idx"]), C.byref(bad))
        return code, o, bad.value

    def close(self):
        self.ctx.close()


ALL = W.WANT_FPT | W.WANT_DWELL | W.WANT_STATS
# name -> (tail, refine, resident references or None); the model of the tail is always resident
COMBOS = {
    "plain+none": (NONE, False, "plain"), "plain+svm": (SVM, False, "svm"), "plain+mlp": (MLP, False, "mlp"),
    "plain+boost+refs": (BOOST, False, "plain"), "plain+boost": (BOOST, False, None),
    "refine+none": (NONE, True, "refine"), "refine+boost": (BOOST, True, None),
}


@functools.lru_cache(maxsize=None)
def _tick_ctx(combo):
    tail, refine, refs_kind = COMBOS[combo]
    refs = {None: None, "plain": _plain_refs, "refine": _refine_refs, "svm": lambda: _svm_model()._X,
            "mlp": lambda: _mlp_model()._X}[refs_kind]
    return Tick(None if refs is None else refs(), svm=_svm_model() if tail == SVM else None,
                mlp=_mlp_model() if tail == MLP else None, boost=_boost_model() if tail == BOOST else None)


def _check(o, e, want, tail, what):
    """every output the tick was asked for equals the yardstick's; what it was not asked for is untouched"""
    asked = {"status", "call"} | ({"fpt"} if want & W.WANT_FPT else set()) | ({"dwell"} if want & W.WANT_DWELL else set())
    asked |= ({"stats"} if want & W.WANT_STATS else set()) | ({"refine_idx"} if want & W.WANT_REFINE_IDX else set())
    asked |= ({"dist"} if want & W.WANT_DIST else set()) | ({"prob", "pred", "conf"} if tail != NONE else set())
    for name in NAMES:
        if name in asked:
            assert _same(o[name], e[name]), f"{what}: {name}"
        else:
            assert (o[name] == -9).all(), f"{what}: {name} was written without being asked for"
    if tail != NONE:
        bad = e["status"] != 0
        assert (o["pred"][bad] == -1).all() and np.isnan(o["prob"][bad]).all() and np.isnan(o["conf"][bad]).all(), what


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt", ["f32", "i16"])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_tick_equals_the_blocking_calls(combo, fmt, n):
    tail, refine, refs_kind = COMBOS[combo]
    t = _tick_ctx(combo)
    e = _yard(fmt, refine, tail, refs_kind, n)
    k = 0 if tail == NONE else e["prob"].shape[1] if n else 4
    want = ALL | (W.WANT_DIST if refs_kind else 0) | (W.WANT_REFINE_IDX if refine else 0)
    if n == 0:     # success, and nothing was touched: the caller's arrays hold room for a read and keep their fill
        code, o, bad = t.run(fmt, 0, tail, refine, want, k=k, room=1)
        assert code == 0, _lib.load().wdx_last_error()
        assert all(v.size > 0 and (v == -9).all() for v in o.values()) and bad == -1
        return
    code, o, bad = t.run(fmt, n, tail, refine, want, k=k)
    assert code == 0, _lib.load().wdx_last_error()
    assert bad == 0
    _check(o, e, want, tail, f"{combo} {fmt} n={n}")
    # asking for less returns the same bits of what is left (the output block is laid out per call)
    code, o, _ = t.run(fmt, n, tail, refine, W.WANT_REFINE_IDX if refine else 0, k=k)
    assert code == 0
    _check(o, e, W.WANT_REFINE_IDX if refine else 0, tail, f"{combo} {fmt} n={n}, status / call / tail only")


@pytest.mark.parametrize("use_svm", [0, 1], ids=["none", "svm"])
def test_live_tick_is_the_float32_plain_corner_of_live_tick_ex(use_svm):
    t = _tick_ctx("plain+svm")
    n, k = 65, _svm_model().n_classes
    code, o, _ = t.run("f32", n, SVM if use_svm else NONE, False, W.WANT_FPT | W.WANT_DIST, k=k)
    assert code == 0
    i = t.inputs("f32", n)
    g = dict(status=np.full(n, -9, np.int32), call=np.full(n, -9, np.int32), dist=np.full((n, t.nY), -9, np.float32),
             fpt=np.full((n, K), -9.0), prob=np.full((n, k), -9.0), pred=np.full(n, -9, np.int32), conf=np.full(n, -9.0))
    pc = _hp().to_c()
    _lib.check(t.L.wdx_live_tick(t.ctx.handle, i["ptrs"], _lib.ptr(i["row_len"]), n, _lib.ptr(i["a_s"]), _lib.ptr(i["a_e"]),
                                 _lib.ptr(i["ok"]), C.byref(pc), t.nY, use_svm, _lib.ptr(g["fpt"]), _lib.ptr(g["dist"]),
                                 _lib.ptr(g["call"]), _lib.ptr(g["status"]), _lib.ptr(g["prob"]), _lib.ptr(g["pred"]),
                                 _lib.ptr(g["conf"])))
    for name, a in g.items():
        assert a.tobytes() == o[name].tobytes(), name
    assert (g["status"] == 0).sum() * 2 >= n and ((g["prob"] == -9).all() if not use_svm else np.isfinite(g["prob"]).any())


def test_refusals_return_their_code_and_leave_the_context_usable():
    L = _lib.load()
    e = _yard("f32", False, BOOST, "plain", 17)
    er = _yard("f32", True, BOOST, None, 17)

    def refused(t, code, *a, **kw):
        got, o, bad = t.run(*a, **kw)
        assert got == code, (got, L.wdx_last_error())
        assert all((v == -9).all() for v in o.values()) and bad == -1, "a refused tick wrote an output"

    full = Tick(_plain_refs(), boost=_boost_model())          # references + boost model; no SVM, no MLP
    bare = Tick(None)                                         # nothing resident
    try:
        def valid():
            code, o, _ = full.run("f32", 17, BOOST, False, ALL | W.WANT_DIST, k=4)
            assert code == 0
            _check(o, e, ALL | W.WANT_DIST, BOOST, "after a refusal")

        for kw in (dict(both_rows=True), dict(no_rows=True)):                          # exactly one of rows / adc_rows
            refused(full, INV, "f32", 17, BOOST, False, 0, k=4, **kw)
            valid()
        for bit in (W.WANT_SVM, W.WANT_BOOST, 0x80):                                   # the tail is `tail`, not a bit
            refused(full, INV, "f32", 17, BOOST, False, bit, k=4)
            valid()
        refused(full, INV, "f32", 17, 4, False, 0, k=4)                                # unknown tail
        refused(full, INV, "f32", 17, BOOST, False, 0, k=4, n_refs=N_REFS + 1)          # dist sized for another set
        refused(full, INV, "f32", 17, BOOST, False, W.WANT_REFINE_IDX, k=4)            # refine_idx without refinement
        refused(full, INV, "f32", 17, BOOST, False, 0, k=4, keep=24)                   # K != the reference length
        valid()
        refused(full, NO_REFS, "f32", 17, SVM, False, 0, k=4)                          # no SVM resident
        refused(full, NO_REFS, "i16", 17, MLP, False, 0, k=4)                          # no MLP resident
        valid()
        refused(full, INV, "f32", 17, SVM, True, 0, k=4)                               # refinement with a DTW tail
        refused(full, INV, "i16", 17, MLP, True, 0, k=4)
        valid()
        # without references: n_refs = 0 serves NONE and BOOST only, and has no distances
        refused(bare, NO_REFS, "f32", 17, BOOST, False, 0, k=4)                        # no boost model
        refused(bare, NO_REFS, "f32", 17, SVM, False, 0, k=4)
        refused(bare, NO_REFS, "f32", 17, MLP, False, 0, k=4)
        refused(bare, NO_REFS, "f32", 17, NONE, False, 0, n_refs=3)
        refused(bare, INV, "f32", 17, NONE, False, W.WANT_DIST)
        code, o, _ = bare.run("i16", 17, NONE, True, ALL | W.WANT_REFINE_IDX)
        assert code == 0
        _check(o, _yard("i16", True, NONE, None, 17), ALL | W.WANT_REFINE_IDX, NONE, "fingerprint-only tick")
        mc = _boost_model().to_c()
        _lib.check(L.wdx_boost_set_model(bare.ctx.handle, C.byref(mc)))
        refused(bare, INV, "f32", 17, BOOST, True, 0, k=4, keep=24)                    # keep != the model's n_features
        refused(bare, INV, "f32", 17, BOOST, False, W.WANT_DIST, k=4)
        mm = _mlp_model().to_c()
        _lib.check(L.wdx_mlp_set_model(bare.ctx.handle, C.byref(mm)))
        refused(bare, NO_REFS, "f32", 17, MLP, False, 0, k=5)                          # an MLP, but no references
        code, o, _ = bare.run("f32", 17, BOOST, True, ALL | W.WANT_REFINE_IDX, k=4)
        assert code == 0
        _check(o, er, ALL | W.WANT_REFINE_IDX, BOOST, "tRNA tick after the refusals")
    finally:
        full.close()
        bare.close()


class ReadObject:   # the fields of live_balancing/utils.py's ReadObject the two workers touch
    def __init__(self, idx, data_arr, polya_start, calibration=None):
        self.idx, self.data_arr, self.polya_start, self.time_per_step, self.is_outlier = idx, data_arr, polya_start, [0.01], None
        self.calibration = calibration


@pytest.mark.parametrize("fmt", ["f32", "i16"])
@pytest.mark.parametrize("kind", ["boost+refine", "mlp"])
def test_demux_worker_with_every_model_kind(kind, fmt):
    n = 17
    b = _batch("worker")
    if kind == "mlp":
        ld = LiveDemux(model=_mlp_model(), params=_hp(), max_reads=20, max_samples=6500, adc=fmt == "i16")
        e = _yard(fmt, False, MLP, "mlp", n, "worker")
    else:
        ld = LiveDemux(model=_boost_model(), params=_hp(), refine=_hr(), max_reads=20, max_samples=6500, adc=fmt == "i16")
        e = _yard(fmt, True, BOOST, None, n, "worker")
    try:
        qin, qout = queue.Queue(), queue.Queue()
        for i in range(n):
            rl = int(b["row_len"][i])
            if fmt == "f32":
                qin.put(ReadObject(i, b["rows"][i, :rl].copy(), int(b["a_e"][i])))
            else:
                qin.put(ReadObject(i, b["adc"][i, :rl].copy(), int(b["a_e"][i]), (float(b["offset"][i]), float(b["scale"][i]))))
        qin.put(None)
        t = threading.Thread(target=demux_worker, args=(qin, qout, ld))
        t.start()
        got = []
        while True:
            o = qout.get(timeout=60)
            if o is None:       # the stop signal is forwarded, last
                break
            got.append(o)
        t.join(10)
        good = np.flatnonzero(e["status"] == 0)
        assert 2 * len(good) >= n and len(good) < n
        assert [o.idx for o in got] == good.tolist()          # failed reads dropped, the others in their order
        for o in got:
            assert o.data_arr.shape == (1, e["prob"].shape[1]) and np.array_equal(o.data_arr[0], e["prob"][o.idx])
            assert o.is_outlier == bool(e["pred"][o.idx] == -1) and len(o.time_per_step) == 3
        # the same reads through the object's own tick: every field, and a float32 tick beside an int16 one
        i = _tick_ctx("plain+none").inputs(fmt, n, "worker")
        args = (i["a_s"], i["a_e"])
        kw = dict(want_fpt=True, want_dwell=True, want_stats=True, want_refine_idx=kind != "mlp")
        r = ld.tick(i["rows"], *args, **kw) if fmt == "f32" else ld.tick_adc(i["rows"], i["offset"], i["scale"], *args, **kw)
        for name in NAMES:
            if getattr(r, name) is not None:
                exp = e[name].astype(np.int64) if name == "pred" else e[name]
                assert _same(getattr(r, name), exp), name
        f = _tick_ctx("plain+none").inputs("f32", n, "worker")
        r2 = ld.tick(f["rows"], f["a_s"], f["a_e"])
        e2 = _yard("f32", kind != "mlp", MLP if kind == "mlp" else BOOST, "mlp" if kind == "mlp" else None, n, "worker")
        assert _same(r2.status, e2["status"]) and _same(r2.prob, e2["prob"]) and _same(r2.conf, e2["conf"])
        # one tick with both kinds of object is refused (the formats differ on a window past the chunk's end)
        qin, qout = queue.Queue(), queue.Queue()
        qin.put(ReadObject(0, b["rows"][0, : b["row_len"][0]].copy(), int(b["a_e"][0])))
        qin.put(ReadObject(1, b["adc"][1, : b["row_len"][1]].copy(), int(b["a_e"][1]), (float(b["offset"][1]), float(b["scale"][1]))))
        qin.put(None)
        with pytest.raises(ValueError, match="int16 and float"):
            demux_worker(qin, qout, ld)
        assert qout.empty()
    finally:
        ld.close()


def test_a_non_finite_mlp_input_raises_what_predict_raises():
    dm = _mlp_model(bad_ref=True)
    i = _tick_ctx("plain+none").inputs("f32", 17)
    X = _fingerprints("f32", False, 17)
    with pytest.raises(ValueError) as want:
        dm.predict(X["fpt"][X["status"] == 0])
    ld = LiveDemux(model=dm, params=_hp(), max_reads=0)
    try:
        with pytest.raises(ValueError) as got:
            ld.tick(i["rows"], i["a_s"], i["a_e"], success=i["ok"])
        assert str(got.value) == str(want.value) and "infinity" in str(got.value)
        # the C ABI itself masks and counts: every read the model was shown is counted, none of the failed ones
        t = Tick(dm._X, mlp=dm)
        code, o, bad = t.run("f32", 17, MLP, False, 0, k=dm.k)
        t.close()
        assert code == 0 and bad == int((X["status"] == 0).sum())
        assert (o["pred"] == -1).all() and np.isnan(o["prob"]).all() and np.isnan(o["conf"]).all()
    finally:
        ld.close()
