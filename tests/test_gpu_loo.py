"""Leave-one-out nearest neighbours of a labelled set on the device (include/wdx.h: wdx_self_nearest_device, wdx_dtw_self_nearest;
parallel_distances.loo_nearest; DemuxEngine.loo_nearest) against the rule restated in NumPy on the oracle's float32 distances
(tests/helpers/loo_rule.py), nn and best bit for bit.

One input per L (helpers.loo_rule.rows): 200 rows -- four chunks of 64, the last partial: 4 diagonal and 6 strictly upper tiles --
with non-members of every kind, mislabelled rows, exact ties at distance 0 on both sides, a label of one row and a row at +inf
from every other (tests/test_loo_host.py shows that the input holds them).  Every row is compared with its OWN entries of the
oracle's matrix.  The reference of a shape is computed once and shared."""
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

from helpers import loo_rule as lr  # noqa: E402
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
TILE_SHAPES = ["short_25_15", "band15_110", "band8_40_3", "band32_110"]
SMALL_N = [1, 2, 63, 64, 65, 129]
FILL = 0x5A5A5A5A   # what an untouched element of an output buffer holds
GUARD = 1024        # elements either side of an output


@functools.lru_cache(maxsize=None)
def _rows(L, n=lr.N_ROWS):
    X, labels, status = lr.rows(L, n)
    for a in (X, labels, status):
        a.setflags(write=False)
    return X, labels, status


@functools.lru_cache(maxsize=None)
def _want(L, window, penalty, n=lr.N_ROWS, with_labels=True, with_status=True):
    X, labels, status = _rows(L, n)
    nn, best = lr.loo_rule(X, labels if with_labels else None, window, penalty, status if with_status else None)
    nn.setflags(write=False), best.setflags(write=False)
    return nn, best


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


def _host_call(L, window, penalty, wide=False, n=lr.N_ROWS):
    _imports()
    X, labels, status = _rows(L, n)
    with _lib.default_context().wide_dtw_for_call(wide):
        return pdist.loo_nearest(X, labels, window, penalty, status=status)


def _assert_same(got, want, what=""):
    (gn, gb), (wn, wb) = got, want
    gn, gb = np.asarray(gn), np.asarray(gb)
    assert gn.dtype == np.int32 and gb.dtype == np.float32 and gn.shape == wn.shape and gb.shape == wb.shape, (what, gn.dtype, gb.dtype, gn.shape, gb.shape)
    bad = np.argwhere((gn != wn) | (lr.bits(gb) != lr.bits(wb)))
    if len(bad):
        a, s = bad[0]
        raise AssertionError("%s: %d of %d cells differ, first at row %d side %d: got nn %d best %r (0x%08x), want nn %d best %r (0x%08x)" % (
            what, len(bad), gn.size, a, s, gn[a, s], gb[a, s], lr.bits(gb)[a, s], wn[a, s], wb[a, s], lr.bits(wb)[a, s]))


# ---- 1: every row is the rule's own ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_nn_and_best_are_the_rules_bit_for_bit(shape):
    L, window, penalty, wide = SHAPES[shape]
    got = _host_call(L, window, penalty, wide)
    nn, best = got
    mem = lr.members(*_rows(L))
    print(shape, "members", int(mem.sum()), "of", len(mem), "rows at +inf", int(np.isposinf(best).all(axis=1).sum()))
    assert int(mem.sum()) == 196 and (nn[~mem] == -1).all() and (lr.bits(best[~mem]) == 0x7FC00000).all()
    assert not np.isnan(best[mem]).any()
    _assert_same(got, _want(L, window, penalty), shape)


@pytest.mark.parametrize("n", SMALL_N)
def test_every_row_at_the_chunk_edges(n):
    """n = 1, 2, 63, 64, 65 and 129 rows on every shape: one partial chunk, one whole chunk, one row into the next, two chunks
    and one row"""
    for shape in sorted(SHAPES):
        L, window, penalty, wide = SHAPES[shape]
        _assert_same(_host_call(L, window, penalty, wide, n), _want(L, window, penalty, n), "%s n = %d" % (shape, n))


# ---- 2: routes and cell forms -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", TILE_SHAPES)
def test_tile_route_equals_general_route(shape):
    _imports()
    L, window, penalty, _ = SHAPES[shape]
    tile = _host_call(L, window, penalty)
    ctx = _lib.default_context()
    with _option(ctx, _lib.OPT_SELF_NEAREST_GENERAL, 1):
        general = _host_call(L, window, penalty)
        small = [_host_call(L, window, penalty, n=n) for n in (2, 65)]
    _assert_same(general, tile, shape + " general vs tile")
    _assert_same(general, _want(L, window, penalty), shape + " general")
    for n, g in zip((2, 65), small):
        _assert_same(g, _want(L, window, penalty, n), "%s general n = %d" % (shape, n))
    for bad in (2, -1):
        with pytest.raises(ValueError, match="WDX_OPT_SELF_NEAREST_GENERAL is 0 or 1, not %d" % bad):
            ctx.set_option(_lib.OPT_SELF_NEAREST_GENERAL, bad)


@pytest.mark.parametrize("mode", [1, 2])
def test_unfused_cells_and_forced_second_pass_give_the_same_bits(mode):
    """WDX_OPT_DTW_UNFUSED 1 (the reference's six operations only) and 2 (every pair settled again) on every tile kernel"""
    _imports()
    ctx = _lib.default_context()
    for shape in TILE_SHAPES:
        L, window, penalty, _ = SHAPES[shape]
        with _option(ctx, _lib.OPT_DTW_UNFUSED, mode):
            got = _host_call(L, window, penalty)
        _assert_same(got, _want(L, window, penalty), "%s unfused %d" % (shape, mode))


def test_no_short_dtw_sends_the_short_shape_to_the_band_kernel():
    _imports()
    L, window, penalty, _ = SHAPES["short_25_15"]
    with _option(_lib.default_context(), _lib.OPT_NO_SHORT_DTW, 1):
        got = _host_call(L, window, penalty)
    _assert_same(got, _want(L, window, penalty), "short shape on the band-15 kernel")


# ---- 3: against the self matrix -------------------------------------------------------------------------------------------------------

def _engine(L, window, penalty, **kw):
    _imports()
    X = _rows(L)[0]
    return DemuxEngine(X[np.isfinite(X).all(axis=1)][:4], window, penalty, **kw)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_equals_the_rule_applied_to_self_distances(shape):
    L, window, penalty, wide = SHAPES[shape]
    X, labels, status = _rows(L)
    eng = _engine(L, window, penalty, wide_dtw=wide)
    try:
        Xd, ld, sd = (torch.from_numpy(a.copy()).cuda() for a in (X, labels, status))
        D = eng.self_distances(Xd, window, penalty, status=sd).cpu().numpy()
        res = eng.loo_nearest(Xd, ld, window=window, penalty=penalty, status=sd)
        got = res.nn.cpu().numpy(), res.best.cpu().numpy()
    finally:
        eng.close()
    _assert_same(got, lr.rule_on_matrix(D, labels, lr.members(X, labels, status)), shape + " vs the rule on self_distances")


# ---- 4: the ways in, the guard bands ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general", [0, 1])
def test_the_ways_in_agree_and_the_device_entry_stays_inside_its_outputs(general):
    """parallel_distances.loo_nearest, wdx_dtw_self_nearest through ctypes, DemuxEngine.loo_nearest and the raw device entry with
    each output between two guard bands of 1 024 elements: the bands keep their fill, X, labels and status are not written;
    without a status array row 195 is a member; without labels the other side is -1 / +inf everywhere"""
    shape = "band8_40_3"
    L, window, penalty, _ = SHAPES[shape]
    X, labels, status = _rows(L)
    n = len(X)
    want = _want(L, window, penalty)
    eng = _engine(L, window, penalty)
    try:
        eng.ctx.set_option(_lib.OPT_SELF_NEAREST_GENERAL, general)
        with _option(_lib.default_context(), _lib.OPT_SELF_NEAREST_GENERAL, general):
            host = pdist.loo_nearest(X, labels, window, penalty, status=status)
        raw_nn, raw_best = np.full((n, 2), FILL, dtype=np.int32), np.full((n, 2), FILL, dtype=np.uint32).view(np.float32)
        _lib.check(eng.L.wdx_dtw_self_nearest(eng.ctx.handle, _lib.ptr(X), n, L, _lib.ptr(labels), _lib.ptr(status), window, penalty,
                                              _lib.ptr(raw_nn), _lib.ptr(raw_best)))
        Xd, ld, sd = (torch.from_numpy(a.copy()).cuda() for a in (X, labels, status))
        X0, l0, s0 = Xd.clone(), ld.clone(), sd.clone()
        res = eng.loo_nearest(Xd, ld, window=window, penalty=penalty, status=sd)
        bn = torch.full((2 * n + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda")
        bb = torch.full((2 * n + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda")
        p = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)   # noqa: E731
        _lib.check(eng.L.wdx_self_nearest_device(eng.ctx.handle, p(Xd), n, L, p(ld), p(sd), window, penalty, p(bn, GUARD), p(bb, GUARD), None))
        bare = eng.loo_nearest(Xd, ld, window=window, penalty=penalty)                 # no status: row 195 is a member
        unlabelled = eng.loo_nearest(Xd, None, window=window, penalty=penalty, status=sd)
        torch.cuda.synchronize()
        assert torch.equal(Xd.view(torch.int64), X0.view(torch.int64)) and torch.equal(ld, l0) and torch.equal(sd, s0), "an input was written"
        dev = []
        for name, buf in (("nn", bn), ("best", bb)):
            b = buf.cpu().numpy().view(np.uint32)
            assert (b[:GUARD] == FILL).all() and (b[GUARD + 2 * n:] == FILL).all(), "a guard band of %s was written" % name
            dev.append(np.ascontiguousarray(b[GUARD:GUARD + 2 * n]).reshape(n, 2))
        dev = dev[0].view(np.int32), dev[1].view(np.float32)
        assert isinstance(res.nn, torch.Tensor) and res.nn.dtype == torch.int32 and res.best.dtype == torch.float32
        eng_out = res.nn.cpu().numpy(), res.best.cpu().numpy()
        bare = bare.nn.cpu().numpy(), bare.best.cpu().numpy()
        unlabelled = unlabelled.nn.cpu().numpy(), unlabelled.best.cpu().numpy()
    finally:
        eng.close()
    for name, got in (("loo_nearest", host), ("wdx_dtw_self_nearest", (raw_nn, raw_best)), ("DemuxEngine.loo_nearest", eng_out),
                      ("wdx_self_nearest_device", dev)):
        _assert_same(got, want, "%s (general %d)" % (name, general))
    _assert_same(bare, _want(L, window, penalty, with_status=False), "without a status array")
    assert bare[0][195, 0] >= 0 and want[0][195, 0] == -1 and np.isnan(want[1][195, 0]) and not np.isnan(bare[1][195, 0])
    _assert_same(unlabelled, _want(L, window, penalty, with_labels=False), "without labels")
    mem = lr.members(X, None, status)
    assert (unlabelled[0][:, 1] == -1).all() and np.isposinf(unlabelled[1][mem, 1]).all() and (unlabelled[0][mem, 0] >= 0).all()


def test_loo_nearest_refuses_what_it_cannot_pass_on():
    L, window, penalty, _ = SHAPES["short_25_15"]
    eng = _engine(L, window, penalty)
    try:
        Xd = torch.from_numpy(_rows(L)[0].copy()).cuda()
        n = Xd.shape[0]
        with pytest.raises(ValueError, match="labels must be a contiguous int32"):
            eng.loo_nearest(Xd, torch.zeros(n, dtype=torch.int64, device="cuda"), window=window, penalty=penalty)
        with pytest.raises(ValueError, match="labels must be a contiguous int32"):
            eng.loo_nearest(Xd, torch.zeros(n - 1, dtype=torch.int32, device="cuda"), window=window, penalty=penalty)
        with pytest.raises(ValueError, match="status must be a contiguous int32"):
            eng.loo_nearest(Xd, None, window=window, penalty=penalty, status=torch.zeros(n, dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError, match="X must be a contiguous float64"):
            eng.loo_nearest(Xd.float(), None, window=window, penalty=penalty)
    finally:
        eng.close()


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------------

def _generation(eng):
    g = C.c_int64(-1)
    _lib.check(eng.L.wdx_refs_generation(eng.ctx.handle, C.byref(g)))
    return g.value


def test_refusals_carry_code_and_message_and_touch_nothing():
    L, window, penalty, _ = SHAPES["short_25_15"]
    X, labels, status = _rows(L)
    eng = _engine(L, window, penalty)
    try:
        Xd, ld, sd = (torch.from_numpy(a.copy()).cuda() for a in (X, labels, status))
        n = len(X)
        nn = torch.full((n, 2), FILL, dtype=torch.int32, device="cuda")
        best = torch.full((n, 2), FILL, dtype=torch.int32, device="cuda")
        gen = _generation(eng)
        before = eng.nearest(Xd).call.cpu().numpy()
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        call = lambda n_, L_, o_nn, o_best: eng.L.wdx_self_nearest_device(eng.ctx.handle, p(Xd), n_, L_, p(ld), None, window, penalty, p(o_nn), p(o_best), None)   # noqa: E731
        err = lambda: eng.L.wdx_last_error().decode()   # noqa: E731
        assert call(n, 0, nn, best) == _lib.WDX_ERR_INVALID and "L must be at least 1, not 0" in err()
        assert call(-1, L, nn, best) == _lib.WDX_ERR_INVALID and "n must not be negative (n = -1)" in err()
        assert call(n, L, None, best) == _lib.WDX_ERR_INVALID and "the outputs nn and best are required" in err()
        assert call(n, L, nn, None) == _lib.WDX_ERR_INVALID and "the outputs nn and best are required" in err()
        big = _lib.SELF_MATRIX_MAX_ROWS + 1
        assert call(big, L, nn, best) == _lib.WDX_ERR_UNSUPPORTED and "n = 65537 rows, more than WDX_SELF_MATRIX_MAX_ROWS = 65536" in err()
        # the host form refuses the same, before it sizes anything
        hn, hb = np.full((4, 2), FILL, dtype=np.int32), np.full((4, 2), FILL, dtype=np.uint32)
        hcall = lambda n_, L_, o_nn, o_best: eng.L.wdx_dtw_self_nearest(eng.ctx.handle, _lib.ptr(X), n_, L_, None, None, window, penalty, o_nn, o_best)   # noqa: E731
        assert hcall(big, L, _lib.ptr(hn), _lib.ptr(hb)) == _lib.WDX_ERR_UNSUPPORTED and "n = 65537 rows" in err()
        assert hcall(4, 0, _lib.ptr(hn), _lib.ptr(hb)) == _lib.WDX_ERR_INVALID and "L must be at least 1" in err()
        assert hcall(4, L, None, _lib.ptr(hb)) == _lib.WDX_ERR_INVALID and "the outputs nn and best are required" in err()
        assert (hn == FILL).all() and (hb == FILL).all()
        with pytest.raises(NotImplementedError, match="n = 65537 rows"):
            eng.loo_nearest(torch.zeros((big, 1), dtype=torch.float64, device="cuda"), None, window=window, penalty=penalty)
        with pytest.raises(NotImplementedError, match="n = 65537 rows"):
            pdist.loo_nearest(np.zeros((big, 1)))
        with pytest.raises(ValueError, match="WDX_OPT_SELF_NEAREST_GENERAL is 0 or 1, not -1"):
            eng.ctx.set_option(_lib.OPT_SELF_NEAREST_GENERAL, -1)
        torch.cuda.synchronize()
        assert (nn.cpu().numpy() == FILL).all() and (best.cpu().numpy() == FILL).all(), "a refused call wrote its outputs"
        # n == 0 is success and writes nothing (with or without outputs)
        assert call(0, L, nn, best) == _lib.WDX_SUCCESS and call(0, L, None, None) == _lib.WDX_SUCCESS and hcall(0, L, None, None) == _lib.WDX_SUCCESS
        empty = eng.loo_nearest(Xd[:0], ld[:0], window=window, penalty=penalty)
        assert tuple(empty.nn.shape) == (0, 2) and tuple(empty.best.shape) == (0, 2)
        hn0, hb0 = pdist.loo_nearest(X[:0], labels[:0], window, penalty)
        assert hn0.shape == (0, 2) and hb0.shape == (0, 2)
        torch.cuda.synchronize()
        assert (nn.cpu().numpy() == FILL).all() and (best.cpu().numpy() == FILL).all(), "an empty call wrote its outputs"
        # nothing resident was touched, and the context still serves
        assert _generation(eng) == gen
        assert np.array_equal(eng.nearest(Xd).call.cpu().numpy(), before)
        res = eng.loo_nearest(Xd, ld, window=window, penalty=penalty, status=sd)
        again = res.nn.cpu().numpy(), res.best.cpu().numpy()
        assert _generation(eng) == gen
        assert np.array_equal(eng.nearest(Xd).call.cpu().numpy(), before)
    finally:
        eng.close()
    _assert_same(again, _want(L, window, penalty), "after the refusals")


# ---- 6: reordering: the merge does not depend on the order of the rows or of the tiles ------------------------------------------------

@pytest.mark.parametrize("shape", ["band15_110", "band8_40_3"])
def test_a_permutation_of_the_rows_gives_the_same_neighbours(shape):
    """rows and labels permuted alike: after the indices are mapped back, best is identical, and nn identical wherever the minimum
    is unique (a tie goes to the lowest index of the order at hand)"""
    _imports()
    L, window, penalty, _ = SHAPES[shape]
    X, labels, status = _rows(L)
    n = len(X)
    nn0, best0 = _want(L, window, penalty)
    perm = np.random.default_rng(5).permutation(n)          # row i of the permuted call is row perm[i]
    nn1, best1 = pdist.loo_nearest(np.ascontiguousarray(X[perm]), labels[perm], window, penalty, status=status[perm])
    back = np.empty(n, dtype=np.int64)
    back[perm] = np.arange(n)
    best_b = best1[back]
    nn_b = np.where(nn1[back] >= 0, perm[np.maximum(nn1[back], 0)], -1)
    assert lr.same_bits(best_b, best0), "%s: best changed under a permutation of the rows" % shape
    # where is the minimum unique?  count the candidates at the minimum on the device's own self matrix
    D = pdist.self_distance_matrix(X, window, penalty, status=status)
    mem = lr.members(X, labels, status)
    unique = np.zeros((n, 2), dtype=bool)
    for a in np.flatnonzero(mem):
        for side, cand in enumerate((mem & (labels == labels[a]) & (np.arange(n) != a), mem & (labels != labels[a]))):
            unique[a, side] = cand.any() and int((D[a, cand] == best0[a, side]).sum()) == 1
    print(shape, "cells with a unique minimum:", int(unique.sum()), "ties:", int((~unique & mem[:, None] & (nn0 >= 0)).sum()))
    assert unique.sum() > 300 and np.array_equal(nn_b[unique], nn0[unique])
    assert ((nn_b >= 0) == (nn0 >= 0)).all()


# ---- 7: the stream contract: enqueued on the caller's stream, no synchronisation -----------------------------------------------------

def test_device_entry_enqueues_on_the_callers_stream_without_waiting():
    """the way tests/test_gpu_self_matrix.py holds wdx_self_matrix_device: on a side stream whose inputs arrive LATE (the tensors
    hold a decoy until, behind a device-side delay, the real rows, labels and status are copied in) the call returns while the
    delay is still running, and gives the serial call's result bit for bit; a fresh child process, which first proves that its
    side streams overtake"""
    res, _ = so.run_child(HERE, ["stream"], timeout=150.0)
    assert res.get("ok") is True and res["same"] and res["pending"] and res["decoy_differs"], res


def _child_stream():
    _imports()
    L, window, penalty, _ = SHAPES["short_25_15"]
    X, labels, status = _rows(L)
    A, B, log = so.side_streams()
    print("\n".join(log))
    eng, ref = _engine(L, window, penalty), _engine(L, window, penalty)
    real = [torch.from_numpy(a.copy()).cuda() for a in (X, labels, status)]
    rng = np.random.default_rng(3)
    decoy = [torch.from_numpy(rng.normal(0, 1, X.shape)).cuda(), torch.from_numpy(rng.integers(0, 5, len(X)).astype(np.int32)).cuda(),
             torch.zeros(len(X), dtype=torch.int32, device="cuda")]
    both = lambda r: np.concatenate([r.nn.cpu().numpy().view(np.uint32), r.best.cpu().numpy().view(np.uint32)], axis=1)   # noqa: E731
    run = lambda e, t: e.loo_nearest(t[0], t[1], window=window, penalty=penalty, status=t[2])   # noqa: E731
    serial = both(run(ref, real))                                                     # default stream, second context
    wrong = both(run(ref, decoy))
    run(eng, real)                                                                    # warm: buffers sized, kernels loaded
    torch.cuda.synchronize()
    t0 = time.time()
    run(eng, real)
    torch.cuda.synchronize()
    ms = so.delay_ms_for(time.time() - t0)
    late = [torch.empty_like(t) for t in real]
    ev = so.late(A, late, real, decoy, ms)
    with torch.cuda.stream(A):
        res = run(eng, late)
        pending = not ev.query()                                                      # the call came back with the delay still running
        got = both(res)                                                               # (copies on A: they wait for A alone)
    same = bool(np.array_equal(got, serial))
    decoy_differs = not np.array_equal(wrong, serial)
    eng.close(), ref.close()
    print(json.dumps(dict(ok=True, same=same, pending=pending, decoy_differs=decoy_differs, delay_ms=ms)))


if __name__ == "__main__":
    if sys.argv[1:] == ["stream"]:
        _child_stream()
