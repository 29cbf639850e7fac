"""The symmetric DTW self-distance matrix on the device (include/wdx.h: wdx_self_matrix_device, wdx_dtw_self_matrix;
parallel_distances.self_distance_matrix; DemuxEngine.self_distances) against the rule restated in NumPy on the oracle's float32
distances (tests/helpers/self_matrix_rule.py), bit for bit -- and models.DTW_SVM.fit on it.

One input per L (helpers.self_matrix_rule.rows): 200 rows -- four chunks of 64, the last partial: 4 diagonal and 6 strictly upper
tiles -- with a NaN row, a row with an infinite sample and a row with status 1.  Every entry is compared with the oracle's OWN
(a, b) entry of the members' matrix, so a device whose f(a, b) differed from f(b, a) would show.  The reference of a shape is
computed once and shared."""
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

from helpers import self_matrix_rule as sr  # noqa: E402
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
FILL = 0x5A5A5A5A   # what an untouched float32 of an output buffer holds


@functools.lru_cache(maxsize=None)
def _rows(L, n=sr.N_ROWS):
    X, status = sr.rows(L, n)
    X.setflags(write=False), status.setflags(write=False)
    return X, status


@functools.lru_cache(maxsize=None)
def _want(L, window, penalty, n=sr.N_ROWS):
    X, status = _rows(L, n)
    D = sr.self_matrix_rule(X, window, penalty, status)
    D.setflags(write=False)
    return D


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


def _host_call(L, window, penalty, wide=False, n=sr.N_ROWS):
    _imports()
    X, status = _rows(L, n)
    with _lib.default_context().wide_dtw_for_call(wide):
        return pdist.self_distance_matrix(X, window, penalty, status=status)


def _assert_same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not sr.same_bits(got, want):
        bad = np.argwhere(sr.bits(got) != sr.bits(want))
        a, b = bad[0]
        raise AssertionError("%s: %d of %d entries differ, first at (%d, %d): got %r (0x%08x), want %r (0x%08x)" % (
            what, len(bad), got.size, a, b, got[a, b], sr.bits(got)[a, b], want[a, b], sr.bits(want)[a, b]))


def _assert_structure(D, L, n):
    """what the input was built to hold: the non-members' rows and columns are the quiet NaN and nothing else is"""
    X, status = _rows(L, n)
    mem = sr.members(X, status)
    nan = sr.bits(D) == 0x7FC00000
    assert np.array_equal(nan, ~(mem[:, None] & mem[None, :])), "the quiet NaN exactly where a row or a column is no member"
    assert not np.isnan(D[np.ix_(mem, mem)]).any()
    return mem


# ---- 1: every entry is the oracle's own -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_entry_is_the_oracles_own_bit_for_bit(shape):
    L, window, penalty, wide = SHAPES[shape]
    got = _host_call(L, window, penalty, wide)
    mem = _assert_structure(got, L, sr.N_ROWS)
    print(shape, "members", int(mem.sum()), "of", len(mem), "max", float(np.nanmax(got)))
    assert int(mem.sum()) == sr.N_ROWS - 3 and not mem[[14, 90, 195]].any()   # a NaN row, an infinite sample, a status: three chunks
    _assert_same(got, _want(L, window, penalty), shape)


@pytest.mark.parametrize("n", SMALL_N)
def test_every_entry_at_the_chunk_edges(n):
    """n = 1, 2, 63, 64, 65 and 129 rows on every shape: one partial chunk, one whole chunk, one row into the next, two chunks
    and one row"""
    for shape in sorted(SHAPES):
        L, window, penalty, wide = SHAPES[shape]
        got = _host_call(L, window, penalty, wide, n)
        _assert_structure(got, L, n)
        _assert_same(got, _want(L, window, penalty, n), "%s n = %d" % (shape, n))


# ---- 2: symmetric, zero diagonal ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_matrix_equals_its_transpose_and_the_members_diagonal_is_zero(shape):
    L, window, penalty, wide = SHAPES[shape]
    got = _host_call(L, window, penalty, wide)
    assert sr.same_bits(got, np.ascontiguousarray(got.T)), "%s: the matrix is not its transpose bit for bit" % shape
    mem = sr.members(*_rows(L))
    assert (sr.bits(np.diag(got))[mem] == 0).all(), "%s: a member's diagonal entry is not +0.0" % shape


# ---- 3: routes and cell forms --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", TILE_SHAPES)
def test_tile_route_equals_general_route(shape):
    _imports()
    L, window, penalty, _ = SHAPES[shape]
    tile = _host_call(L, window, penalty)
    ctx = _lib.default_context()
    with _option(ctx, _lib.OPT_SELF_MATRIX_GENERAL, 1):
        general = _host_call(L, window, penalty)
        small = [_host_call(L, window, penalty, n=n) for n in (2, 65)]
    _assert_same(general, tile, shape + " general vs tile")
    _assert_same(general, _want(L, window, penalty), shape + " general")
    for n, g in zip((2, 65), small):
        _assert_same(g, _want(L, window, penalty, n), "%s general n = %d" % (shape, n))
    with pytest.raises(ValueError, match="WDX_OPT_SELF_MATRIX_GENERAL is 0 or 1"):
        ctx.set_option(_lib.OPT_SELF_MATRIX_GENERAL, 2)


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


# ---- 4: the existing matrix entry ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_equals_the_existing_dtw_matrix_of_the_members(shape):
    _imports()
    L, window, penalty, wide = SHAPES[shape]
    X, status = _rows(L)
    mem = sr.members(X, status)
    M = np.ascontiguousarray(X[mem])
    with _lib.default_context().wide_dtw_for_call(wide):
        old = pdist.distance_matrix_to(M, M, window=window, penalty=penalty, n_jobs=1)
    got = _host_call(L, window, penalty, wide)
    _assert_same(np.ascontiguousarray(got[np.ix_(mem, mem)]), old, shape + " vs wdx_dtw_matrix(M, M)")


# ---- 5: the ways in, the leading dimension, the guard bands -------------------------------------------------------------------------

GUARD = 1024   # elements either side of the output


def _engine(L, window, penalty, **kw):
    _imports()
    X = _rows(L)[0]
    return DemuxEngine(X[np.isfinite(X).all(axis=1)][:4], window, penalty, **kw)


@pytest.mark.parametrize("general", [0, 1])
def test_the_ways_in_agree_and_the_device_entry_stays_inside_its_output(general):
    """wdx_dtw_self_matrix through ctypes (with ld = n + 37 on the host), parallel_distances.self_distance_matrix,
    DemuxEngine.self_distances (plain, and into a wider tensor), and the raw device entry with ld = n + 37 between two guard
    bands of 1 024 elements: the gap columns and the bands keep their fill, X and status are not written"""
    shape = "band8_40_3"
    L, window, penalty, _ = SHAPES[shape]
    X, status = _rows(L)
    n, ld = len(X), len(X) + 37
    want = _want(L, window, penalty)
    eng = _engine(L, window, penalty)
    try:
        eng.ctx.set_option(_lib.OPT_SELF_MATRIX_GENERAL, general)
        _lib.default_context().set_option(_lib.OPT_SELF_MATRIX_GENERAL, general)
        try:
            host = pdist.self_distance_matrix(X, window, penalty, status=status)
        finally:
            _lib.default_context().set_option(_lib.OPT_SELF_MATRIX_GENERAL, 0)
        raw = np.full((n, ld), FILL, dtype=np.uint32).view(np.float32)
        _lib.check(eng.L.wdx_dtw_self_matrix(eng.ctx.handle, _lib.ptr(X), n, L, _lib.ptr(status), window, penalty, _lib.ptr(raw), ld))
        Xd, sd = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(status.copy()).cuda()
        X0, s0 = Xd.clone(), sd.clone()
        plain = eng.self_distances(Xd, window, penalty, status=sd)
        wide = torch.full((n, ld), FILL, dtype=torch.int32, device="cuda").view(torch.float32)
        view = eng.self_distances(Xd, window, penalty, status=sd, out=wide)
        assert view.data_ptr() == wide.data_ptr() and tuple(view.shape) == (n, n)
        buf = torch.full((n * ld + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda")
        _lib.check(eng.L.wdx_self_matrix_device(eng.ctx.handle, C.c_void_p(Xd.data_ptr()), n, L, C.c_void_p(sd.data_ptr()), window, penalty,
                                                C.c_void_p(buf.data_ptr() + GUARD * 4), ld, None))
        # ... and without a status array: row 195 is a member then
        bare = eng.self_distances(Xd, window, penalty)
        torch.cuda.synchronize()
        assert torch.equal(Xd.view(torch.int64), X0.view(torch.int64)) and torch.equal(sd, s0), "an input was written"
        b = buf.cpu().numpy().view(np.uint32)
        assert (b[:GUARD] == FILL).all() and (b[GUARD + n * ld:] == FILL).all(), "a guard band was written"
        dev = b[GUARD:GUARD + n * ld].reshape(n, ld)
        assert (dev[:, n:] == FILL).all(), "the device entry wrote into the gap columns"
        w = wide.cpu().numpy().view(np.uint32)
        assert (w[:, n:] == FILL).all(), "self_distances wrote into the gap columns of a wider tensor"
        assert (raw.view(np.uint32)[:, n:] == FILL).all(), "the host form wrote into the gap columns"
        plain, bare = plain.cpu().numpy(), bare.cpu().numpy()
    finally:
        eng.close()
    for name, got in (("self_distance_matrix", host), ("wdx_dtw_self_matrix", np.ascontiguousarray(raw[:, :n])),
                      ("DemuxEngine.self_distances", plain), ("self_distances(out=wider)", np.ascontiguousarray(w[:, :n]).view(np.float32)),
                      ("wdx_self_matrix_device", np.ascontiguousarray(dev[:, :n]).view(np.float32))):
        _assert_same(got, want, "%s (general %d)" % (name, general))
    _assert_same(bare, sr.self_matrix_rule(X, window, penalty), "without a status array")
    assert not np.isnan(bare[195, 0]) and np.isnan(want[195, 0])


def test_self_distances_refuses_what_it_cannot_pass_on():
    L, window, penalty, _ = SHAPES["short_25_15"]
    eng = _engine(L, window, penalty)
    try:
        Xd = torch.from_numpy(_rows(L)[0].copy()).cuda()
        n = Xd.shape[0]
        for bad in (torch.empty((n, n - 1), dtype=torch.float32, device="cuda"), torch.empty((n, n), dtype=torch.float64, device="cuda"),
                    torch.empty((n + 1, n), dtype=torch.float32, device="cuda"), torch.empty((n, 2 * n), dtype=torch.float32, device="cuda")[:, ::2]):
            with pytest.raises(ValueError, match="out must be a float32 device tensor of 200 rows"):
                eng.self_distances(Xd, window, penalty, out=bad)
        with pytest.raises(ValueError, match="status must be a contiguous int32"):
            eng.self_distances(Xd, window, penalty, status=torch.zeros(n, dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError, match="X must be a contiguous float64"):
            eng.self_distances(Xd.float(), window, penalty)
    finally:
        eng.close()


# ---- 7: refusals --------------------------------------------------------------------------------------------------------------------

def _generation(eng):
    g = C.c_int64(-1)
    _lib.check(eng.L.wdx_refs_generation(eng.ctx.handle, C.byref(g)))
    return g.value


def test_refusals_carry_code_and_message_and_touch_nothing():
    L, window, penalty, _ = SHAPES["short_25_15"]
    X, status = _rows(L)
    eng = _engine(L, window, penalty)
    try:
        Xd = torch.from_numpy(X.copy()).cuda()
        n = len(X)
        out = torch.full((n, n), FILL, dtype=torch.int32, device="cuda")
        gen = _generation(eng)
        before = eng.nearest(Xd).call.cpu().numpy()
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        call = lambda n_, L_, ld_, o: eng.L.wdx_self_matrix_device(eng.ctx.handle, p(Xd), n_, L_, None, window, penalty, p(o), ld_, None)   # noqa: E731
        err = lambda: eng.L.wdx_last_error().decode()   # noqa: E731
        assert call(n, 0, n, out) == _lib.WDX_ERR_INVALID and "L must be at least 1, not 0" in err()
        assert call(-1, L, n, out) == _lib.WDX_ERR_INVALID and "n must not be negative (n = -1)" in err()
        assert call(n, L, n - 1, out) == _lib.WDX_ERR_INVALID and "ld = 199 is less than n = 200" in err()
        assert call(n, L, n, None) == _lib.WDX_ERR_INVALID and "the output matrix is required" in err()
        big = _lib.SELF_MATRIX_MAX_ROWS + 1
        assert call(big, L, big, out) == _lib.WDX_ERR_UNSUPPORTED and "n = 65537 rows, more than WDX_SELF_MATRIX_MAX_ROWS = 65536" in err()
        # the host form refuses the same, before it allocates anything
        host = np.full((4, 4), FILL, dtype=np.uint32)
        hcall = lambda n_, L_, ld_, o: eng.L.wdx_dtw_self_matrix(eng.ctx.handle, _lib.ptr(X), n_, L_, None, window, penalty, o, ld_)   # noqa: E731
        assert hcall(big, L, big, _lib.ptr(host)) == _lib.WDX_ERR_UNSUPPORTED and "n = 65537 rows" in err()
        assert hcall(4, L, 3, _lib.ptr(host)) == _lib.WDX_ERR_INVALID and "ld = 3 is less than n = 4" in err()
        assert hcall(4, L, 4, None) == _lib.WDX_ERR_INVALID and "the output matrix is required" in err()
        assert (host == FILL).all()
        with pytest.raises(NotImplementedError, match="n = 65537 rows"):
            eng.self_distances(torch.zeros((big, 1), dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError, match="WDX_OPT_SELF_MATRIX_GENERAL is 0 or 1, not -1"):
            eng.ctx.set_option(_lib.OPT_SELF_MATRIX_GENERAL, -1)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == FILL).all(), "a refused call wrote its output"
        # n == 0 is success and writes nothing (with or without an output)
        assert call(0, L, 0, out) == _lib.WDX_SUCCESS and call(0, L, 0, None) == _lib.WDX_SUCCESS and hcall(0, L, 0, None) == _lib.WDX_SUCCESS
        assert tuple(eng.self_distances(Xd[:0], window, penalty).shape) == (0, 0)
        assert pdist.self_distance_matrix(X[:0], window, penalty).shape == (0, 0)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == FILL).all(), "an empty call wrote its output"
        # nothing resident was touched, and the context still serves
        assert _generation(eng) == gen
        assert np.array_equal(eng.nearest(Xd).call.cpu().numpy(), before)
        again = eng.self_distances(Xd, window, penalty, status=torch.from_numpy(status.copy()).cuda()).cpu().numpy()
        assert _generation(eng) == gen
        assert np.array_equal(eng.nearest(Xd).call.cpu().numpy(), before)
    finally:
        eng.close()
    _assert_same(again, _want(L, window, penalty), "after the refusals")


# ---- 6: the stream contract: enqueued on the caller's stream, no synchronisation ---------------------------------------------------

def test_device_entry_enqueues_on_the_callers_stream_without_waiting():
    """the way tests/test_gpu_medoids.py holds wdx_medoids_device: on a side stream whose inputs arrive LATE (the tensors hold a
    decoy until, behind a device-side delay, the real rows and status are copied in) the call returns while the delay is still
    running, and gives the serial call's matrix bit for bit; a fresh child process, which first proves that its side streams
    overtake"""
    res, _ = so.run_child(HERE, ["stream"], timeout=150.0)
    assert res.get("ok") is True and res["same"] and res["pending"] and res["decoy_differs"], res


def _child_stream():
    _imports()
    L, window, penalty, _ = SHAPES["short_25_15"]
    X, status = _rows(L)
    A, B, log = so.side_streams()
    print("\n".join(log))
    eng, ref = _engine(L, window, penalty), _engine(L, window, penalty)
    real = [torch.from_numpy(X.copy()).cuda(), torch.from_numpy(status.copy()).cuda()]
    rng = np.random.default_rng(3)
    decoy = [torch.from_numpy(rng.normal(0, 1, X.shape)).cuda(), torch.zeros(len(X), dtype=torch.int32, device="cuda")]
    serial = ref.self_distances(real[0], window, penalty, status=real[1]).cpu().numpy()          # default stream, second context
    wrong = ref.self_distances(decoy[0], window, penalty, status=decoy[1]).cpu().numpy()
    eng.self_distances(real[0], window, penalty, status=real[1])                                   # warm: buffers sized, kernels loaded
    torch.cuda.synchronize()
    t0 = time.time()
    eng.self_distances(real[0], window, penalty, status=real[1])
    torch.cuda.synchronize()
    ms = so.delay_ms_for(time.time() - t0)
    Xt, st = torch.empty_like(real[0]), torch.empty_like(real[1])
    ev = so.late(A, [Xt, st], real, decoy, ms)
    with torch.cuda.stream(A):
        res = eng.self_distances(Xt, window, penalty, status=st)
        pending = not ev.query()                                                     # the call came back with the delay still running
        got = res.cpu().numpy()                                                      # (a copy on A: it waits for A alone)
    same = sr.same_bits(got, serial)
    decoy_differs = not sr.same_bits(wrong, serial)
    eng.close(), ref.close()
    print(json.dumps(dict(ok=True, same=same, pending=pending, decoy_differs=decoy_differs, delay_ms=ms)))


# ---- 8: fit on the device ------------------------------------------------------------------------------------------------------------

FITS = {"5x300_L25": (5, 300, 25, 3), "4x200_L110": (4, 200, 110, 4)}   # classes, training rows, L, seed; window 15, penalty 0.1


@pytest.mark.parametrize("case", sorted(FITS))
def test_fit_on_the_device_is_the_svc_on_the_oracles_kernel(case):
    """`DTW_SVM.fit` takes its training matrix from the device; the distances are the oracle's bit for bit, so libsvm sees the same
    input and the fitted arrays equal, exactly, those of an SVC with the same random_state fitted on the oracle's kernel.
    `predict` on 256 held-out rows then matches that SVC's predict_proba on the oracle's kernel rows to 1e-5 (the bar of
    tests/test_gpu_live.py and DESIGN.md 2), every read included: first the coupling's stopping margin of all 256 is shown to be at
    least 1e-5 on the CPU reference (tests/helpers/svm_ref.py)."""
    from sklearn.svm import SVC

    from helpers import svm_ref
    from oracle import wdx_oracle as orc
    from warpdemux_amd.models import DTW_SVM

    k, n_train, L, seed = FITS[case]
    window, penalty = 15, 0.1
    Xtr, y, Xte, yte = sr.training_rows(k, n_train, L, seed)
    labels = np.arange(k) * 3 + 2                    # non-contiguous barcode numbers
    model = DTW_SVM.fit(Xtr, labels[y], window, penalty)
    D = orc.dtw_matrix(Xtr, Xtr, window, penalty)
    svc = SVC(kernel="precomputed", probability=True, C=1.0, random_state=0).fit(np.exp(-1.0 * np.power(D, 1)), labels[y])
    sp = orc.svm_params(svc)
    for name, g, w in zip(("n_support", "support", "dual_coef", "rho", "probA", "probB"),
                          (model._n_support, model._support, model._dual_coef, model._rho, model._probA, model._probB), sp[:6]):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), "%s: %s differs from the SVC on the oracle's kernel" % (case, name)
    assert model.label_mapper == {i: int(c) for i, c in enumerate(labels)} and model.n_dropped_ == 0 and np.array_equal(model._X, Xtr)
    Kq = np.exp(-orc.dtw_matrix(Xte, Xtr, window, penalty))
    ref = svm_ref.predict(Kq, *sp[:6])
    print(case, "smallest stopping margin", float(ref.margin.min()))
    assert (ref.margin >= 1e-5).all(), "a held-out read sits on the coupling's stopping boundary: change the generator"
    want_prob = svc.predict_proba(Kq)
    y_pred, y_prob = model.predict(Xte, nproc=1)
    err = float(np.abs(y_prob - want_prob).max())
    print(case, "max |prob - predict_proba|", err, "accuracy", float((y_pred == labels[yte]).mean()))
    assert err <= 1e-5
    assert np.array_equal(y_pred, svc.classes_[np.argmax(want_prob, axis=1)])
    assert np.array_equal(y_pred, labels[yte])      # (accuracy 1.0 on these generators, checked on the CPU reference)


def test_fit_drops_non_members_on_the_device_path():
    from oracle import wdx_oracle as orc
    from warpdemux_amd.models import DTW_SVM

    k, n_train, L, seed = FITS["5x300_L25"]
    Xtr, y, _, _ = sr.training_rows(k, n_train, L, seed)
    X = Xtr.copy()
    X[5, 3] = np.nan
    status = np.zeros(n_train, dtype=np.int32)
    status[250] = 1
    keep = np.ones(n_train, dtype=bool)
    keep[[5, 250]] = False
    model = DTW_SVM.fit(X, y, 15, 0.1, status=status)
    D = orc.dtw_matrix(Xtr[keep], Xtr[keep], 15, 0.1)
    want = DTW_SVM.fit(Xtr[keep], y[keep], 15, 0.1, distances=D)
    assert model.n_dropped_ == 2 and np.array_equal(model._X, Xtr[keep])
    assert np.array_equal(model._dual_coef, want._dual_coef) and np.array_equal(model._support, want._support)
    assert np.array_equal(model._probA, want._probA) and np.array_equal(model._rho, want._rho)


if __name__ == "__main__":
    if sys.argv[1:] == ["stream"]:
        _child_stream()
