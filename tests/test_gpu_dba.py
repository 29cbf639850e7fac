"""One barycenter step on the device (include/wdx.h: wdx_dba_step_device, wdx_dtw_dba_step; parallel_distances.dba_step,
label_barycenters; DemuxEngine.dba_step, barycenters) against the rule restated in NumPy (tests/helpers/dba_rule.py), bit for bit:
the new centres, the counts, the inertia, every row's cost and every row's alignment (the runs), so that a wrong path and a wrong
sum can be told apart.

The input of every shape is helpers.medoid_rule.labelled_rows(L): labels of 1, 2, 63, 64, 65, 129 and 200 rows in shuffled row
order, an empty label, rows labelled -1, a NaN row, a row with an infinite sample, a row with status 1, a label whose only row has
status 1.  The centres are the rule's medoids, with the centre of label 3 set to NaN (idle by its centre).  The reference of a shape
is computed once and shared."""
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

from helpers import dba_rule as dr  # noqa: E402
from helpers import medoid_rule as mr  # noqa: E402
from helpers import stream_order as so  # noqa: E402

pytestmark = pytest.mark.gpu

# name: (L, window, penalty)
SHAPES = {
    "band_25_15": (25, 15, 0.1),
    "band15_exact_110": (110, 15, 0.1),
    "band8_40": (40, 8, 0.1),
    "band16_one_word_33": (33, 16, 0),
    "band32_two_words_70": (70, 32, 0.1),
    "short_5_masked_rows": (5, 15, 0.1),
    "single_point": (1, 1, 0),
    "general_unbanded_40": (40, None, 0),
    "general_110_40": (110, 40, 0.1),
}
BAND = ["band_25_15", "band15_exact_110", "band8_40", "band16_one_word_33", "band32_two_words_70", "short_5_masked_rows", "single_point"]
KEYS = ("runs", "cost", "new_centres", "count", "inertia")
IDLE_BY_CENTRE = 3


@functools.lru_cache(maxsize=None)
def _rows(L):
    return mr.labelled_rows(L)


@functools.lru_cache(maxsize=None)
def _centres(L, window, penalty):
    X, lab, status, G = _rows(L)
    Cm = mr.medoid_rule(X, lab, G, window, penalty, status)["refs"].copy()
    Cm[IDLE_BY_CENTRE, L // 2] = np.nan
    return Cm


@functools.lru_cache(maxsize=None)
def _want(L, window, penalty):
    X, lab, status, G = _rows(L)
    return dr.dba_step(X, lab, _centres(L, window, penalty), G, window, penalty, status)


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


def _as_dict(t):
    return dict(zip(("new_centres", "count", "inertia", "cost", "runs"), t))


def _host_call(L, window, penalty):
    _imports()
    X, lab, status, G = _rows(L)
    return _as_dict(pdist.dba_step(X, lab, _centres(L, window, penalty), G, window, penalty, status=status, want_cost=True, want_runs=True))


def _assert_same(got, want, what="", keys=KEYS):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if not mr.same_bits(g, w):
            assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
            bad = np.flatnonzero((mr.bits(g) != mr.bits(w)).reshape(len(g), -1).any(axis=1))
            raise AssertionError("%s %s: %d of %d differ, first at %s: got %r, want %r" % (what, k, bad.size, len(g), bad[:5], g[bad[:2]], w[bad[:2]]))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_output_is_the_rule_bit_for_bit(shape):
    L, window, penalty = SHAPES[shape]
    X, lab, status, G = _rows(L)
    want = _want(L, window, penalty)
    got = _host_call(L, window, penalty)
    print(shape, "counts", got["count"].tolist(), "inertia", got["inertia"].tolist())
    _assert_same(got, want, shape)
    # the input holds what the issue names: idle by members (7, 8), idle by centre (3), non-members of three kinds
    assert got["count"].tolist() == [1, 2, 63, 0, 64, 128, 199, 0, 0]
    idle = [IDLE_BY_CENTRE, 7, 8]
    assert np.isnan(got["new_centres"][idle]).all() and np.isnan(got["inertia"][idle]).all() and np.isfinite(got["new_centres"][[0, 1, 2, 4, 5, 6]]).all()
    assert np.isnan(got["cost"]).sum() == 6 + 4 + 64 and (got["runs"][np.isnan(got["cost"])] == -1).all()
    lo, hi = got["runs"][~np.isnan(got["cost"])].transpose(2, 0, 1)
    assert (lo[:, 0] == 0).all() and (hi[:, -1] == L - 1).all() and (hi[:, :-1] <= lo[:, 1:]).all() and (lo[:, 1:] <= hi[:, :-1] + 1).all()


@pytest.mark.parametrize("penalty", [0, 0.5])
@pytest.mark.parametrize("general", [0, 1])
def test_ties_between_predecessors_go_the_rules_way(penalty, general):
    """rows and centres drawn from {-1, 0, 1}: equal predecessors abound (tests/test_dba_host.py checks that at least a tenth of the
    path steps of this input sit on a tied cell)"""
    _imports()
    L, window = 40, 8
    X, lab, Cm, G = dr.tied_input(L)
    want = dr.dba_step(X, lab, Cm, G, window, penalty)
    with _option(_lib.default_context(), _lib.OPT_DBA_GENERAL, general):
        got = _as_dict(pdist.dba_step(X, lab, Cm, G, window, penalty, want_cost=True, want_runs=True))
    _assert_same(got, want, "ties, penalty %r, general %d" % (penalty, general))


@pytest.mark.parametrize("shape", BAND)
def test_general_route_equals_band_route(shape):
    _imports()
    L, window, penalty = SHAPES[shape]
    band = _host_call(L, window, penalty)
    ctx = _lib.default_context()
    with _option(ctx, _lib.OPT_DBA_GENERAL, 1):
        general = _host_call(L, window, penalty)
    _assert_same(general, band, shape + " general vs band")
    _assert_same(general, _want(L, window, penalty), shape + " general")
    with pytest.raises(ValueError, match="WDX_OPT_DBA_GENERAL is 0 or 1, not 2"):
        ctx.set_option(_lib.OPT_DBA_GENERAL, 2)


@pytest.mark.parametrize("shape", ["band15_exact_110", "general_unbanded_40"])
def test_rooted_cost_is_the_shipped_distance(shape):
    _imports()
    L, window, penalty = SHAPES[shape]
    X, lab, status, G = _rows(L)
    Cm = _centres(L, window, penalty)
    cost = _host_call(L, window, penalty)["cost"]
    for g in range(G):
        q = np.flatnonzero((lab == g) & ~np.isnan(cost))
        if q.size:
            D = pdist.distance_matrix_to(X[q], Cm[g:g + 1], window=window, penalty=penalty, n_jobs=1)[:, 0]
            assert mr.same_bits(np.sqrt(cost[q]).astype(np.float32), D), (shape, g)


def test_a_call_of_two_passes_equals_its_rows_taken_alone():
    """L 1 024 unbanded: 32 direction words per row, 256 KiB of codes per lane, so the 256 MiB code block holds 1 024 lanes and the
    1 152 padded rows of this call take two launches -- the second with row0 = 1 024, 128 lanes on the stride of 1 024, the last chunk
    of label 0 and label 1 in it.  Every row's cost and runs must be what single-pass calls on parts of the rows return (those kernels
    are held to the rule at the small shapes), and the centres, counts and inertia what the rule's averaging makes of these runs."""
    _imports()
    L, penalty = 1024, 0.1
    rng = np.random.default_rng(5)
    lab = np.r_[np.zeros(1030, dtype=np.int32), np.ones(40, dtype=np.int32)]
    rng.shuffle(lab)
    base = np.cumsum(rng.normal(0, 0.3, (2, L)), axis=1)
    X = base[lab] + rng.normal(0, 0.3, (lab.size, L))
    Cm = base + rng.normal(0, 0.1, (2, L))
    padded = sum(-(-int((lab == g).sum()) // 64) * 64 for g in (0, 1))
    assert padded == 1152 and (256 << 20) // (L * 32 * 8) == 1024 < padded, "the shape must need two passes"
    new, count, inertia, cost, runs = pdist.dba_step(X, lab, Cm, 2, None, penalty, want_cost=True, want_runs=True)
    q0, q1 = np.flatnonzero(lab == 0), np.flatnonzero(lab == 1)
    for part, g in ((q0[:600], 0), (q0[600:], 0), (q1, 1)):
        alone = pdist.dba_step(X[part], np.zeros(part.size, dtype=np.int32), Cm[g:g + 1], 1, None, penalty, want_cost=True, want_runs=True)
        assert mr.same_bits(cost[part], alone[3]) and mr.same_bits(runs[part], alone[4]), g
    assert count.tolist() == [1030, 40]
    for g, q in ((0, q0), (1, q1)):
        lo, hi = runs[q, :, 0], runs[q, :, 1]
        want_new, want_inertia = dr.average(dr.run_sums(X[q], lo, hi), lo, hi, cost[q], np.arange(q.size), q.size)
        assert mr.same_bits(new[g], want_new) and inertia[g] == want_inertia, g


def test_a_label_beyond_the_medoids_cap_is_served():
    """a step has no block that grows with the square of a label: WDX_MEDOID_MAX_GROUP does not apply"""
    _imports()
    L, window, penalty = 5, 3, 0.1
    rng = np.random.default_rng(9)
    n = _lib.MEDOID_MAX_GROUP + 70
    X = rng.normal(0, 1, (n, L))
    lab = np.zeros(n, dtype=np.int32)
    Cm = rng.normal(0, 1, (1, L))
    got = _as_dict(pdist.dba_step(X, lab, Cm, 1, window, penalty, want_cost=True, want_runs=True))
    _assert_same(got, dr.dba_step(X, lab, Cm, 1, window, penalty), "33 000 rows of one label")
    assert got["count"].tolist() == [n]


def test_loop_is_three_rule_steps_and_stops_at_a_fixed_point():
    _imports()
    L, window, penalty = SHAPES["band8_40"]
    X, lab, status, G = _rows(L)
    init = pdist.label_medoids(X, lab, G, window, penalty, status=status)[1]
    want = dr.barycenters(X, lab, init, G, window, penalty, status, n_iter=3)
    got = pdist.label_barycenters(X, lab, G, window, penalty, status=status, n_iter=3)
    assert want[2].shape == (3, G)
    for name, g, w in zip(("centres", "count", "inertia"), got, want):
        assert mr.same_bits(g, w), name
    # a label of identical rows whose samples are multiples of 1/16 (every sum and quotient exact) is a fixed point of its own row
    row = np.round(X[np.flatnonzero(lab == 6)[0]] * 16) / 16
    Xf = np.tile(row, (70, 1))
    centres, count, inertia = pdist.label_barycenters(Xf, np.zeros(70, dtype=np.int32), 1, window, penalty, init=row[None], n_iter=5)
    assert inertia.shape == (1, 1) and inertia[0, 0] == 0.0 and count.tolist() == [70] and mr.same_bits(centres, row[None])


def _engine(L, window, penalty, **kw):
    _imports()
    X = _rows(L)[0]
    return DemuxEngine(X[np.isfinite(X).all(axis=1)][:4], window, penalty, **kw)


def _np_result(res):
    return dict(new_centres=res.centres.cpu().numpy(), count=res.count.cpu().numpy(), inertia=res.inertia.cpu().numpy(),
                cost=None if res.cost is None else res.cost.cpu().numpy(), runs=None if res.runs is None else res.runs.cpu().numpy())


def _generation(eng):
    g = C.c_int64(-1)
    _lib.check(eng.L.wdx_refs_generation(eng.ctx.handle, C.byref(g)))
    return g.value


def test_engine_entry_agrees_and_nothing_resident_changes():
    L, window, penalty = SHAPES["band8_40"]
    X, lab, status, G = _rows(L)
    eng = _engine(L, window, penalty)
    try:
        Xd, sd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(status).cuda(), torch.from_numpy(_centres(L, window, penalty)).cuda()
        gen = _generation(eng)
        before = eng.dtw(Xd)[0].cpu().numpy()
        got = _np_result(eng.dba_step(Xd, lab, Cd, G, window=window, penalty=penalty, status=sd, want_cost=True, want_runs=True))
        bare = _np_result(eng.dba_step(Xd, lab, Cd, window=window, penalty=penalty, status=sd))
        centres, count, inertia = eng.barycenters(Xd, lab, G, window=window, penalty=penalty, status=sd, n_iter=2)
        assert _generation(eng) == gen and mr.same_bits(eng.dtw(Xd)[0].cpu().numpy(), before)
        loop = [t.cpu().numpy() for t in (centres, count, inertia)]
    finally:
        eng.close()
    _assert_same(got, _want(L, window, penalty), "DemuxEngine.dba_step")
    assert bare["cost"] is None and bare["runs"] is None
    _assert_same(bare, got, "without the nullable outputs", keys=("new_centres", "count", "inertia"))
    init = mr.medoid_rule(X, lab, G, window, penalty, status)["refs"]
    for name, g, w in zip(("centres", "count", "inertia"), loop, dr.barycenters(X, lab, init, G, window, penalty, status, n_iter=2)):
        assert mr.same_bits(g, w), name


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_carry_code_and_message_and_write_nothing():
    L, window, penalty = SHAPES["band_25_15"]
    X, lab, status, G = _rows(L)
    eng = _engine(L, window, penalty)
    try:
        Xd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(_centres(L, window, penalty)).cuda()
        n = len(X)
        out = torch.full((G * 1025,), -7.0, dtype=torch.float64, device="cuda")
        cnt = torch.full((G,), -7, dtype=torch.int64, device="cuda")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        call = lambda X_, n_, L_, lab_, G_, C_, new: eng.L.wdx_dba_step_device(eng.ctx.handle, p(X_), n_, L_, _lib.ptr(lab_), G_, None, p(C_), window,
                                                                             penalty, p(new), p(cnt), None, None, None, None)
        err = lambda: eng.L.wdx_last_error().decode()
        assert call(Xd, n, L, lab, 0, Cd, out) == _lib.WDX_ERR_INVALID and "n_labels must be at least 1, not 0" in err()
        bad = lab.copy()
        bad[17] = G
        assert call(Xd, n, L, bad, G, Cd, out) == _lib.WDX_ERR_INVALID and "the label of row 17 is %d, outside -1 .. %d" % (G, G - 1) in err()
        assert call(Xd, n, 0, lab, G, Cd, out) == _lib.WDX_ERR_INVALID and "L must be at least 1, not 0" in err()
        assert call(Xd, -1, L, lab, G, Cd, out) == _lib.WDX_ERR_INVALID
        assert call(Xd, n, L, lab, G, Cd, None) == _lib.WDX_ERR_INVALID and call(Xd, n, L, lab, G, None, out) == _lib.WDX_ERR_INVALID
        Xlong = torch.zeros((4, 1025), dtype=torch.float64, device="cuda")
        Clong = torch.zeros((G, 1025), dtype=torch.float64, device="cuda")
        assert call(Xlong, 4, 1025, lab[:4], G, Clong, out) == _lib.WDX_ERR_UNSUPPORTED and "L = 1025" in err() and "WDX_DBA_MAX_L = 1024" in err()
        with pytest.raises(NotImplementedError, match="L = 1025"):
            eng.dba_step(Xlong, lab[:4], Clong, G, window=window, penalty=penalty)
        with pytest.raises(ValueError, match="lie in -1 .. 8"):
            eng.dba_step(Xd, bad, Cd, G, window=window, penalty=penalty)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7.0).all() and (cnt.cpu().numpy() == -7).all(), "a refused call wrote its output"
        # an empty batch is success with every label idle
        empty = eng.dba_step(Xd[:0], lab[:0], Cd, G, window=window, penalty=penalty, want_cost=True, want_runs=True)
        assert torch.isnan(empty.centres).all() and empty.count.tolist() == [0] * G and torch.isnan(empty.inertia).all()
        assert empty.cost.numel() == 0 and empty.runs.numel() == 0
        # the context still serves
        again = _np_result(eng.dba_step(Xd, lab, Cd, G, window=window, penalty=penalty, status=torch.from_numpy(status).cuda(), want_cost=True,
                                        want_runs=True))
    finally:
        eng.close()
    _assert_same(again, _want(L, window, penalty), "after the refusals")


# ---- the device entry stays inside its outputs -----------------------------------------------------------------------------------

GUARD = 1024   # elements either side of every output


@pytest.mark.parametrize("general", [0, 1])
@pytest.mark.parametrize("nullable", [True, False])
def test_device_entry_writes_nothing_outside_its_outputs(general, nullable):
    L, window, penalty = SHAPES["band8_40"]
    X, lab, status, G = _rows(L)
    n = len(X)
    want = _want(L, window, penalty)
    eng = _engine(L, window, penalty)
    try:
        eng.ctx.set_option(_lib.OPT_DBA_GENERAL, general)
        Xd, sd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(status).cuda(), torch.from_numpy(_centres(L, window, penalty)).cuda()
        X0, s0, C0 = Xd.clone(), sd.clone(), Cd.clone()
        sizes = dict(new_centres=(G * L, torch.float64), count=(G, torch.int64), inertia=(G, torch.float64), cost=(n, torch.float64),
                     runs=(n * L * 2, torch.int32))
        if not nullable:
            sizes = dict(new_centres=sizes["new_centres"])
        words = {k: (m * torch.empty(0, dtype=dt).element_size() + 7) // 8 for k, (m, dt) in sizes.items()}
        buf = {k: torch.full((words[k] + 2 * GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda") for k in sizes}
        ptr = {k: C.c_void_p(buf[k].data_ptr() + GUARD * 8) for k in sizes}
        _lib.check(eng.L.wdx_dba_step_device(eng.ctx.handle, C.c_void_p(Xd.data_ptr()), n, L, _lib.ptr(lab), G, C.c_void_p(sd.data_ptr()),
                                             C.c_void_p(Cd.data_ptr()), window, penalty, ptr["new_centres"], ptr.get("count"), ptr.get("inertia"),
                                             ptr.get("cost"), ptr.get("runs"), None))
        torch.cuda.synchronize()
        got = {}
        for k, (m, dt) in sizes.items():
            raw = buf[k].cpu().numpy()
            assert (raw[:GUARD] == 0x5A5A5A5A5A5A5A5A).all() and (raw[GUARD + words[k]:] == 0x5A5A5A5A5A5A5A5A).all(), "%s: a guard band was written" % k
            got[k] = buf[k][GUARD:GUARD + words[k]].view(dt)[:m].cpu().numpy()
        got["new_centres"] = got["new_centres"].reshape(G, L)
        if nullable:
            got["runs"] = got["runs"].reshape(n, L, 2)
        assert torch.equal(Xd.view(torch.int64), X0.view(torch.int64)) and torch.equal(sd, s0) and torch.equal(Cd.view(torch.int64), C0.view(torch.int64)), \
            "an input was written"
    finally:
        eng.close()
    _assert_same(got, want, "guarded outputs", keys=KEYS if nullable else ("new_centres",))


# ---- the stream contract: enqueued on the caller's stream, no synchronisation ---------------------------------------------------

def test_device_entry_enqueues_on_the_callers_stream_without_waiting():
    """the way tests/test_gpu_medoids.py holds wdx_medoids_device: on a side stream whose inputs arrive LATE (the tensors hold a decoy
    until, behind a device-side delay, the real rows, status and centres are copied in) the call returns while the delay is still
    running, and gives the serial call's results bit for bit; a fresh child process, which first proves that its side streams overtake"""
    res, _ = so.run_child(HERE, ["stream"], timeout=150.0)
    assert res.get("ok") is True and res["same"] and res["pending"] and res["decoy_differs"], res


def _child_stream():
    _imports()
    L, window, penalty = SHAPES["band_25_15"]
    X, lab, status, G = _rows(L)
    A, B, log = so.side_streams()
    print("\n".join(log))
    eng, ref = _engine(L, window, penalty), _engine(L, window, penalty)
    real = [torch.from_numpy(X).cuda(), torch.from_numpy(status).cuda(), torch.from_numpy(_centres(L, window, penalty)).cuda()]
    rng = np.random.default_rng(3)
    decoy = [torch.from_numpy(rng.normal(0, 1, X.shape)).cuda(), torch.zeros(len(X), dtype=torch.int32, device="cuda"),
             torch.from_numpy(rng.normal(0, 1, (G, L))).cuda()]
    kw = dict(window=window, penalty=penalty, want_cost=True, want_runs=True)
    serial = _np_result(ref.dba_step(real[0], lab, real[2], G, status=real[1], **kw))     # default stream, second context
    wrong = _np_result(ref.dba_step(decoy[0], lab, decoy[2], G, status=decoy[1], **kw))
    eng.dba_step(real[0], lab, real[2], G, status=real[1], **kw)                          # warm: buffers sized, kernels loaded
    torch.cuda.synchronize()
    t0 = time.time()
    eng.dba_step(real[0], lab, real[2], G, status=real[1], **kw)
    torch.cuda.synchronize()
    ms = so.delay_ms_for(time.time() - t0)
    Xt, st, Ct = torch.empty_like(real[0]), torch.empty_like(real[1]), torch.empty_like(real[2])
    ev = so.late(A, [Xt, st, Ct], real, decoy, ms)
    with torch.cuda.stream(A):
        res = eng.dba_step(Xt, lab, Ct, G, status=st, **kw)
        pending = not ev.query()                                                         # the call came back with the delay still running
        got = _np_result(res)                                                            # (copies on A: they wait for A alone)
    same = all(mr.same_bits(got[k], serial[k]) for k in serial)
    decoy_differs = not mr.same_bits(wrong["cost"], serial["cost"])
    eng.close(), ref.close()
    print(json.dumps(dict(ok=True, same=same, pending=pending, decoy_differs=decoy_differs, delay_ms=ms)))


if __name__ == "__main__":
    if sys.argv[1:] == ["stream"]:
        _child_stream()
