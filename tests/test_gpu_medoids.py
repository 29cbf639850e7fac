"""Per-label DTW medoids on the device (include/wdx.h: wdx_medoids_device, wdx_dtw_medoids; parallel_distances.label_medoids;
DemuxEngine.medoids) against the rule restated in NumPy on the oracle's float32 distances (tests/helpers/medoid_rule.py), bit for bit.

One input serves every shape (helpers.medoid_rule.labelled_rows): labels of 1, 2, 63, 64, 65, 129 and 200 rows in shuffled row order,
one empty label, rows labelled -1, a NaN row, a row with an infinite sample, a row with status 1, and a label whose only row has
status 1 (no member).  Every row's cost is compared with sums taken from that row's OWN oracle distances, so a device whose
f(a, b) differed from f(b, a) would show.  The reference of a shape is computed once and shared."""
import ctypes as C
import contextlib
import functools
import json
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.abspath(__file__)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import medoid_rule as mr  # noqa: E402
from helpers import stream_order as so  # noqa: E402

pytestmark = pytest.mark.gpu

# name: (L, window, penalty, wide_dtw) -- the unrolled short form | the band ladder 15 exact / 8 / 32 | the general route
SHAPES = {
    "short_25_15": (25, 15, 0.1, False),
    "band15_110": (110, 15, 0.1, False),
    "band8_40_3": (40, 3, 1.5, False),
    "band32_110": (110, 32, 0.1, False),
    "unbanded_110_scratch": (110, None, 0.1, False),
    "unbanded_110_wide": (110, None, 0.1, True),
}


@functools.lru_cache(maxsize=None)
def _rows(L):
    return mr.labelled_rows(L)


@functools.lru_cache(maxsize=None)
def _want(L, window, penalty):
    X, lab, status, G = _rows(L)
    return mr.medoid_rule(X, lab, G, window, penalty, status)


def _imports():
    global torch, _lib, pdist, DemuxEngine
    import torch
    from warpdemux_amd import _lib, parallel_distances as pdist
    from warpdemux_amd.engine import DemuxEngine


@contextlib.contextmanager
def _option(ctx, opt, value):
    ctx.set_option(opt, value)
    try:
        yield
    finally:
        ctx.set_option(opt, 0)


def _host_call(L, window, penalty, wide=False):
    _imports()
    X, lab, status, G = _rows(L)
    with _lib.default_context().wide_dtw_for_call(wide):
        index, refs, count, mcost, cost = pdist.label_medoids(X, lab, G, window, penalty, status=status, want_cost=True)
    return dict(index=index, refs=refs, count=count, medoid_cost=mcost, cost=cost)


def _assert_same(got, want, what=""):
    for k in ("cost", "index", "count", "medoid_cost", "refs"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if not mr.same_bits(g, w):
            bad = np.flatnonzero((mr.bits(g) != mr.bits(w)).reshape(len(g), -1).any(axis=1))
            raise AssertionError("%s %s: %d of %d differ, first at %s: got %r, want %r" % (what, k, bad.size, len(g), bad[:5], g[bad[:3]], w[bad[:3]]))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_costs_medoids_counts_and_refs_are_the_rule_bit_for_bit(shape):
    L, window, penalty, wide = SHAPES[shape]
    X, lab, status, G = _rows(L)
    want = _want(L, window, penalty)
    got = _host_call(L, window, penalty, wide)
    print(shape, "medoids", got["index"].tolist(), "counts", got["count"].tolist())
    _assert_same(got, want, shape)
    # the input holds what the issue names: labels without a member, non-members of three kinds, more than one chunk
    assert got["index"][7] == -1 and got["index"][8] == -1 and got["count"].tolist() == [1, 2, 63, 64, 64, 128, 199, 0, 0]
    assert np.isnan(got["refs"][7]).all() and np.isnan(got["refs"][8]).all() and np.isnan(got["medoid_cost"][[7, 8]]).all()
    assert np.isnan(got["cost"][lab == -1]).all() and np.isnan(got["cost"]).sum() == 6 + 4
    assert mr.same_bits(got["refs"][:7], X[got["index"][:7]])


@pytest.mark.parametrize("shape", ["band15_110", "short_25_15", "unbanded_110_wide"])
def test_equal_costs_go_to_the_earlier_row(shape):
    """one label whose two central rows are identical: on the oracle their costs are the two smallest and equal; the device picks
    the earlier row"""
    _imports()
    L, window, penalty, wide = SHAPES[shape]
    X, lab, G, first, second = mr.tied_rows(L, window, penalty)
    want = mr.medoid_rule(X, lab, G, window, penalty)
    q = np.flatnonzero(lab == 0)
    order = q[np.argsort(want["cost"][q], kind="stable")]
    assert first < second and mr.same_bits(X[first], X[second]) and {order[0], order[1]} == {first, second}
    assert want["cost"][first] == want["cost"][second] <= want["cost"][order[2]], "the oracle's two smallest costs must tie"
    with _lib.default_context().wide_dtw_for_call(wide):
        index, refs, count, mcost, cost = pdist.label_medoids(X, lab, G, window, penalty, want_cost=True)
    assert index[0] == first and want["index"][0] == first and mcost[0] == want["cost"][second]
    _assert_same(dict(index=index, refs=refs, count=count, medoid_cost=mcost, cost=cost), want, shape + " tie")


@pytest.mark.parametrize("shape", ["short_25_15", "band15_110", "band8_40_3", "band32_110"])
def test_tile_route_equals_general_route(shape):
    _imports()
    L, window, penalty, _ = SHAPES[shape]
    tile = _host_call(L, window, penalty)
    ctx = _lib.default_context()
    with _option(ctx, _lib.OPT_MEDOID_GENERAL, 1):
        general = _host_call(L, window, penalty)
    _assert_same(general, tile, shape + " general vs tile")
    _assert_same(general, _want(L, window, penalty), shape + " general")
    with pytest.raises(ValueError, match="WDX_OPT_MEDOID_GENERAL is 0 or 1"):
        ctx.set_option(_lib.OPT_MEDOID_GENERAL, 2)


@pytest.mark.parametrize("mode", [1, 2])
def test_unfused_cells_and_forced_second_pass_give_the_same_bits(mode):
    """WDX_OPT_DTW_UNFUSED 1 (the reference's six operations only) and 2 (every pair settled again) on the band-8 and the short shape"""
    _imports()
    ctx = _lib.default_context()
    for shape in ("band8_40_3", "short_25_15"):
        L, window, penalty, _ = SHAPES[shape]
        with _option(ctx, _lib.OPT_DTW_UNFUSED, mode):
            got = _host_call(L, window, penalty)
        _assert_same(got, _want(L, window, penalty), "%s unfused %d" % (shape, mode))


def _engine(L, window, penalty, **kw):
    _imports()
    X = _rows(L)[0]
    return DemuxEngine(X[np.isfinite(X).all(axis=1)][:4], window, penalty, **kw)


def _np_result(res):
    return dict(index=res.index.cpu().numpy(), refs=res.refs.cpu().numpy(), count=res.count.cpu().numpy(),
                medoid_cost=res.medoid_cost.cpu().numpy(), cost=None if res.cost is None else res.cost.cpu().numpy())


def test_the_three_ways_in_agree():
    """wdx_dtw_medoids through ctypes, parallel_distances.label_medoids and DemuxEngine.medoids"""
    L, window, penalty, _ = SHAPES["band8_40_3"]
    X, lab, status, G = _rows(L)
    want = _want(L, window, penalty)
    host = _host_call(L, window, penalty)
    eng = _engine(L, window, penalty)
    try:
        res = eng.medoids(torch.from_numpy(X).cuda(), lab, G, window=window, penalty=penalty, status=torch.from_numpy(status).cuda(),
                          want_cost=True)
        dev = _np_result(res)
        n = len(X)
        raw = dict(index=np.empty(G, np.int64), refs=np.empty((G, L)), count=np.empty(G, np.int64), medoid_cost=np.empty(G), cost=np.empty(n))
        _lib.check(eng.L.wdx_dtw_medoids(eng.ctx.handle, _lib.ptr(X), n, L, _lib.ptr(lab), G, _lib.ptr(status), window, penalty,
                                         _lib.ptr(raw["index"]), _lib.ptr(raw["medoid_cost"]), _lib.ptr(raw["count"]), _lib.ptr(raw["cost"]),
                                         _lib.ptr(raw["refs"])))
        # ... and with every nullable output left out, and no status
        bare = np.empty(G, np.int64)
        _lib.check(eng.L.wdx_dtw_medoids(eng.ctx.handle, _lib.ptr(X), n, L, _lib.ptr(lab), G, None, window, penalty, _lib.ptr(bare), None,
                                         None, None, None))
        no_status = eng.medoids(torch.from_numpy(X).cuda(), lab, window=window, penalty=penalty)
        assert no_status.cost is None and np.array_equal(no_status.index.cpu().numpy(), bare)
    finally:
        eng.close()
    for name, got in (("label_medoids", host), ("DemuxEngine.medoids", dev), ("wdx_dtw_medoids", raw)):
        _assert_same(got, want, name)
    assert bare[8] >= 0 and bare[6] >= 0    # (without the status array label 8's row is a member)


def test_medoids_as_the_reference_set_call_themselves():
    """labelled rows -> medoids -> set_refs -> nearest: every medoid row is called with its own label at distance 0"""
    L, window, penalty, _ = SHAPES["short_25_15"]
    X, lab, status, G = _rows(L)
    eng = _engine(L, window, penalty)
    try:
        Xd = torch.from_numpy(X).cuda()
        res = eng.medoids(Xd, lab, G, window=window, penalty=penalty, status=torch.from_numpy(status).cuda())
        have = (res.index >= 0).cpu().numpy()
        assert have.tolist() == [True] * 7 + [False, False]
        eng.set_refs(res.refs[torch.from_numpy(have).cuda()], window, penalty)      # the labels without a member have NaN rows: left out
        near = eng.nearest(Xd, labels=np.flatnonzero(have).astype(np.int32), n_labels=G)
        call, best, index = near.call.cpu().numpy(), near.best.cpu().numpy(), res.index.cpu().numpy()
    finally:
        eng.close()
    for g in np.flatnonzero(have):
        assert call[index[g]] == g and best[index[g], 0] == 0.0, (g, index[g], call[index[g]], best[index[g]])


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def _generation(eng):
    g = C.c_int64(-1)
    _lib.check(eng.L.wdx_refs_generation(eng.ctx.handle, C.byref(g)))
    return g.value


def test_refusals_carry_code_and_message_and_touch_nothing_resident():
    L, window, penalty, _ = SHAPES["short_25_15"]
    X, lab, status, G = _rows(L)
    eng = _engine(L, window, penalty)
    try:
        Xd = torch.from_numpy(X).cuda()
        n = len(X)
        out = torch.full((G,), -7, dtype=torch.int64, device="cuda")
        gen = _generation(eng)
        before = eng.nearest(Xd).call.cpu().numpy()
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        call = lambda n_, L_, lab_, G_, med: eng.L.wdx_medoids_device(eng.ctx.handle, p(Xd), n_, L_, _lib.ptr(lab_), G_, None, window, penalty,
                                                                    p(med), None, None, None, None, None)
        err = lambda: eng.L.wdx_last_error().decode()
        assert call(n, L, lab, 0, out) == _lib.WDX_ERR_INVALID and "n_labels must be at least 1, not 0" in err()
        bad = lab.copy()
        bad[17] = G
        assert call(n, L, bad, G, out) == _lib.WDX_ERR_INVALID and "the label of row 17 is %d, outside -1 .. %d" % (G, G - 1) in err()
        bad[17] = -2
        assert call(n, L, bad, G, out) == _lib.WDX_ERR_INVALID and "the label of row 17 is -2" in err()
        assert call(n, 0, lab, G, out) == _lib.WDX_ERR_INVALID and "L must be at least 1, not 0" in err()
        assert call(n, L, lab, G, None) == _lib.WDX_ERR_INVALID and "medoid output is required" in err()
        big = np.zeros(_lib.MEDOID_MAX_GROUP + 1 + 3, dtype=np.int32)
        big[:3] = 1
        Xbig = torch.zeros((len(big), L), dtype=torch.float64, device="cuda")
        rc = eng.L.wdx_medoids_device(eng.ctx.handle, p(Xbig), len(big), L, _lib.ptr(big), 2, None, window, penalty, p(out), None, None, None,
                                      None, None)
        assert rc == _lib.WDX_ERR_UNSUPPORTED and "label 0 has 32769 rows, more than WDX_MEDOID_MAX_GROUP = 32768" in err()
        with pytest.raises(NotImplementedError, match="label 0 has 32769 rows"):
            eng.medoids(Xbig, big, window=window, penalty=penalty)
        with pytest.raises(ValueError, match="lie in -1 .. 8"):
            eng.medoids(Xd, bad, G, window=window, penalty=penalty)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7).all(), "a refused call wrote its output"
        # an empty batch is success
        empty = eng.medoids(Xd[:0], lab[:0], 3, window=window, penalty=penalty, want_cost=True)
        assert empty.index.tolist() == [-1, -1, -1] and empty.count.tolist() == [0, 0, 0] and empty.cost.numel() == 0
        assert torch.isnan(empty.refs).all() and torch.isnan(empty.medoid_cost).all()
        # nothing resident was touched, and the context still serves
        assert _generation(eng) == gen
        assert np.array_equal(eng.nearest(Xd).call.cpu().numpy(), before)
        again = _np_result(eng.medoids(Xd, lab, G, window=window, penalty=penalty, status=torch.from_numpy(status).cuda(), want_cost=True))
        assert _generation(eng) == gen
    finally:
        eng.close()
    _assert_same(again, _want(L, window, penalty), "after the refusals")


# ---- the device entry stays inside its outputs -----------------------------------------------------------------------------------

GUARD = 1024   # elements either side of every output


@pytest.mark.parametrize("general", [0, 1])
def test_device_entry_writes_nothing_outside_its_outputs(general):
    L, window, penalty, _ = SHAPES["band8_40_3"]
    X, lab, status, G = _rows(L)
    n = len(X)
    want = _want(L, window, penalty)
    eng = _engine(L, window, penalty)
    try:
        eng.ctx.set_option(_lib.OPT_MEDOID_GENERAL, general)
        Xd, sd = torch.from_numpy(X).cuda(), torch.from_numpy(status).cuda()
        X0, s0 = Xd.clone(), sd.clone()
        sizes = dict(index=(G, torch.int64), medoid_cost=(G, torch.float64), count=(G, torch.int64), cost=(n, torch.float64),
                     refs=(G * L, torch.float64))
        buf = {k: torch.full((m + 2 * GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda").view(dt) for k, (m, dt) in sizes.items()}
        ptr = {k: C.c_void_p(buf[k].data_ptr() + GUARD * 8) for k in sizes}
        _lib.check(eng.L.wdx_medoids_device(eng.ctx.handle, C.c_void_p(Xd.data_ptr()), n, L, _lib.ptr(lab), G, C.c_void_p(sd.data_ptr()), window,
                                            penalty, ptr["index"], ptr["medoid_cost"], ptr["count"], ptr["cost"], ptr["refs"], None))
        torch.cuda.synchronize()
        got = {}
        for k, (m, dt) in sizes.items():
            raw = buf[k].view(torch.int64).cpu().numpy()
            assert (raw[:GUARD] == 0x5A5A5A5A5A5A5A5A).all() and (raw[GUARD + m:] == 0x5A5A5A5A5A5A5A5A).all(), "%s: a guard band was written" % k
            got[k] = buf[k][GUARD:GUARD + m].cpu().numpy()
        got["refs"] = got["refs"].reshape(G, L)
        assert torch.equal(Xd.view(torch.int64), X0.view(torch.int64)) and torch.equal(sd, s0), "an input was written"
    finally:
        eng.close()
    _assert_same(got, want, "guarded outputs")


# ---- the stream contract: enqueued on the caller's stream, no synchronisation ---------------------------------------------------

def test_device_entry_enqueues_on_the_callers_stream_without_waiting():
    """the way tests/test_gpu_streams.py holds wdx_nearest_dev: on a side stream whose inputs arrive LATE (the tensors hold a decoy
    until, behind a device-side delay, the real rows and status are copied in) the call returns while the delay is still running,
    and gives the serial call's results bit for bit; a fresh child process, which first proves that its side streams overtake"""
    res, _ = so.run_child(HERE, ["stream"], timeout=150.0)
    assert res.get("ok") is True and res["same"] and res["pending"] and res["decoy_differs"], res


def _child_stream():
    _imports()
    L, window, penalty, _ = SHAPES["short_25_15"]
    X, lab, status, G = _rows(L)
    A, B, log = so.side_streams()
    print("\n".join(log))
    eng, ref = _engine(L, window, penalty), _engine(L, window, penalty)
    real = [torch.from_numpy(X).cuda(), torch.from_numpy(status).cuda()]
    rng = np.random.default_rng(3)
    decoy = [torch.from_numpy(rng.normal(0, 1, X.shape)).cuda(), torch.zeros(len(X), dtype=torch.int32, device="cuda")]
    kw = dict(window=window, penalty=penalty, want_cost=True)
    serial = _np_result(ref.medoids(real[0], lab, G, status=real[1], **kw))          # default stream, second context
    wrong = _np_result(ref.medoids(decoy[0], lab, G, status=decoy[1], **kw))
    eng.medoids(real[0], lab, G, status=real[1], **kw)                               # warm: buffers sized, kernels loaded
    torch.cuda.synchronize()
    t0 = time.time()
    eng.medoids(real[0], lab, G, status=real[1], **kw)
    torch.cuda.synchronize()
    ms = so.delay_ms_for(time.time() - t0)
    Xt, st = torch.empty_like(real[0]), torch.empty_like(real[1])
    ev = so.late(A, [Xt, st], real, decoy, ms)
    with torch.cuda.stream(A):
        res = eng.medoids(Xt, lab, G, status=st, **kw)
        pending = not ev.query()                                                     # the call came back with the delay still running
        got = _np_result(res)                                                        # (copies on A: they wait for A alone)
    same = all(mr.same_bits(got[k], serial[k]) for k in serial)
    decoy_differs = not mr.same_bits(wrong["cost"], serial["cost"])
    eng.close(), ref.close()
    print(json.dumps(dict(ok=True, same=same, pending=pending, decoy_differs=decoy_differs, delay_ms=ms)))


if __name__ == "__main__":
    if sys.argv[1:] == ["stream"]:
        _child_stream()
