"""The one-wave-per-tile DTW kernels (medoid_tile_kernel, self_tile_kernel, loo_tile_kernel) over the edge table of
tests/helpers/tile_edges.py: every kernel of the register-band ladder at the ends of its windows, every joint of the window-15 row
schedule, windows larger than L, L = 1 and 2, penalty 0, and rows so small that their distances are float32 denormals or exactly
+0.0 -- through the host-array entries (parallel_distances.label_medoids, self_distance_matrix, loo_nearest), at
WDX_OPT_DTW_UNFUSED 0, 1 and 2, bit for bit against the rule helpers on the oracle's float32 matrix.

Every row is compared with its OWN oracle entries (no symmetry is assumed: the self and leave-one-out kernels compute each unordered
pair once).  An expectation is computed once per (input, window, penalty) and shared between the modes, the routes and -- the self
matrix and leave-one-out read one input -- the two families.  tests/test_tile_edges_host.py holds what the table and the inputs
are, and that no row of the table is left out here."""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import loo_rule as lr  # noqa: E402
from helpers import medoid_rule as mr  # noqa: E402
from helpers import self_matrix_rule as sr  # noqa: E402
from helpers import tile_edges as te  # noqa: E402

pytestmark = pytest.mark.gpu

EDGE_CASES = sorted((f, r) for f in te.FAMILIES for r in te.EDGES)
BAND16_ROWS = sorted(r for r in te.EDGES if te.row_kernel(r) == "band16")
RAN = set()   # the (family, row, mode) cases this session has run and found right


def _imports():
    global _lib, pdist, oracle_dtw
    from helpers.dtw_cases import oracle_dtw
    from warpdemux_amd import _lib, parallel_distances as pdist


@contextlib.contextmanager
def _options(**values):
    """WDX_OPT_* by name for the duration of the block; every one of them back to 0 behind it, whatever happened inside"""
    ctx = _lib.default_context()
    opts = [(getattr(_lib, "OPT_" + k), v) for k, v in values.items() if v]
    try:
        for opt, v in opts:
            ctx.set_option(opt, v)
        yield
    finally:
        for opt, _ in opts:
            ctx.set_option(opt, 0)


GENERAL_OPTION = {"medoids": "MEDOID_GENERAL", "self_matrix": "SELF_MATRIX_GENERAL", "loo": "SELF_NEAREST_GENERAL"}


# ---- the expectations: once per (input, window, penalty) ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _want_matrix(L, window, penalty, n):
    _imports()
    X, labels, status = te.loo_input(L, n)
    D = sr.self_matrix_rule(X, window, penalty, status, matrix=lambda A, B: oracle_dtw(A, B, window, penalty))
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def _want_loo(L, window, penalty, n):
    X, labels, status = te.loo_input(L, n)
    # the members of leave-one-out are members of the self matrix: the rule reads their entries of it alone
    nn, best = lr.rule_on_matrix(_want_matrix(L, window, penalty, n), labels, lr.members(X, labels, status))
    nn.setflags(write=False), best.setflags(write=False)
    return nn, best


@functools.lru_cache(maxsize=None)
def _want_medoids(L, window, penalty):
    _imports()
    X, labels, status, G = te.medoid_input(L)
    return mr.medoid_rule(X, labels, G, window, penalty, status, matrix=lambda A: oracle_dtw(A, A, window, penalty))


def _want(family, row, n=lr.N_ROWS):
    L, window, penalty = te.EDGES[row]
    if family == "medoids":
        return _want_medoids(L, window, penalty)
    return (_want_matrix if family == "self_matrix" else _want_loo)(L, window, penalty, n)


# ---- the device calls ----------------------------------------------------------------------------------------------------------------

def _call(family, row, mode=0, general=False, n=lr.N_ROWS):
    _imports()
    L, window, penalty = te.EDGES[row]
    options = {"DTW_UNFUSED": mode, "NO_SHORT_DTW": int(row in te.NO_SHORT), GENERAL_OPTION[family]: int(general)}
    with _options(**options):
        if family == "medoids":
            X, labels, status, G = te.medoid_input(L)
            index, refs, count, mcost, cost = pdist.label_medoids(X, labels, G, window, penalty, status=status, want_cost=True)
            return dict(index=index, refs=refs, count=count, medoid_cost=mcost, cost=cost)
        X, labels, status = te.loo_input(L, n)
        if family == "self_matrix":
            return pdist.self_distance_matrix(X, window, penalty, status=status)
        return pdist.loo_nearest(X, labels, window, penalty, status=status)


def _assert_same(family, got, want, what):
    if family == "medoids":
        for k in ("cost", "index", "count", "medoid_cost", "refs"):
            g, w = np.asarray(got[k]), np.asarray(want[k])
            if not mr.same_bits(g, w):
                bad = np.flatnonzero((mr.bits(g) != mr.bits(w)).reshape(len(g), -1).any(axis=1))
                raise AssertionError("%s %s: %d of %d differ, first at %s: got %r, want %r" % (what, k, bad.size, len(g), bad[:5], g[bad[:3]], w[bad[:3]]))
    elif family == "self_matrix":
        got = np.asarray(got)
        assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
        bad = np.argwhere(sr.bits(got) != sr.bits(want))
        if len(bad):
            a, b = bad[0]
            raise AssertionError("%s: %d of %d entries differ, first at (%d, %d): got %r (0x%08x), want %r (0x%08x)" % (
                what, len(bad), got.size, a, b, got[a, b], sr.bits(got)[a, b], want[a, b], sr.bits(want)[a, b]))
    else:
        (gn, gb), (wn, wb) = got, want
        gn, gb = np.asarray(gn), np.asarray(gb)
        assert gn.dtype == np.int32 and gb.dtype == np.float32 and gn.shape == wn.shape and gb.shape == wb.shape, (what, gn.dtype, gb.dtype)
        bad = np.argwhere((gn != wn) | (lr.bits(gb) != lr.bits(wb)))
        if len(bad):
            a, s = bad[0]
            raise AssertionError("%s: %d of %d cells differ, first at row %d side %d: got nn %d best %r (0x%08x), want nn %d best %r (0x%08x)" % (
                what, len(bad), gn.size, a, s, gn[a, s], gb[a, s], lr.bits(gb)[a, s], wn[a, s], wb[a, s], lr.bits(wb)[a, s]))


def _assert_small_rows(family, row, got, what):
    """what the small rows must give, said by name (the bit comparison holds all of it already)"""
    L = te.EDGES[row][0]
    if family == "medoids":
        X, labels, status, G = te.medoid_input(L)
        mem = np.isfinite(X).all(axis=1) & (labels >= 0) & (status == 0)
        cost = got["cost"]
        assert not np.isnan(cost[mem]).any() and not (mr.bits(cost[mem]) >> 63).any(), what + ": a member's cost is NaN or negative"
        assert np.isnan(cost[~mem]).all()
        return
    X, labels, status = te.loo_input(L)
    den, zero, tiny = te.small_rows(*lr.rows(L))
    if family == "self_matrix":
        mem = sr.members(X, status)
        D = got[np.ix_(mem, mem)]
        assert not np.isnan(D).any(), what + ": NaN between members"
        assert not (sr.bits(D) >> 31).any(), what + ": a sign bit between members"
        z = np.concatenate([zero, tiny])
        assert (sr.bits(got[np.ix_(z, z)]) == 0).all(), what + ": the zero rows are not at +0.0 from each other"
        block = got[np.ix_(den, den)][~np.eye(len(den), dtype=bool)]
        assert ((block > 0) & (block < np.float32(2.0 ** -126))).all(), what + ": the 1e-41 rows are not at denormal distances"
        return
    nn, best = got
    mem = lr.members(X, labels, status)
    assert not np.isnan(best[mem]).any(), what + ": a member's best is NaN"
    assert not (lr.bits(best) >> 31).any(), what + ": a best has its sign bit set"
    for a, side, b in te.zero_neighbours(labels, zero):
        assert nn[a, side] == b and lr.bits(best)[a, side] == 0, "%s: 1e-170 row %d side %d: nn %d best %r, not row %d at +0.0" % (
            what, a, side, nn[a, side], best[a, side], b)
    d = best[den]
    assert ((d > 0) & (d < np.float32(2.0 ** -126))).all(), what + ": a 1e-41 row's best is no denormal"


# ---- 1: every row of the table, every family, the three cell modes --------------------------------------------------------------------

@pytest.mark.parametrize("family,row", EDGE_CASES, ids=["%s-%s" % c for c in EDGE_CASES])
def test_every_output_is_the_rules_bit_for_bit(family, row):
    want = _want(family, row)
    for mode in te.MODES:
        got = _call(family, row, mode)
        what = "%s %s %s unfused %d" % (family, row, te.row_kernel(row), mode)
        _assert_small_rows(family, row, got, what)
        _assert_same(family, got, want, what)
        RAN.add((family, row, mode))
    print("%s %s: kernel %s%s, modes %s" % (family, row, te.row_kernel(row),
          (" schedule %r" % (te.schedule_of(te.EDGES[row][0]),)) if te.row_kernel(row) == "band15" else "", list(te.MODES)))


# ---- 2: the band16 kernels at the chunk edges ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["self_matrix", "loo"])
@pytest.mark.parametrize("row", BAND16_ROWS)
def test_band16_rows_at_the_chunk_edges(family, row):
    """n = 1, 2, 63, 64, 65 and 129 rows: one partial chunk, one whole chunk, one row into the next, two chunks and one row"""
    assert len(BAND16_ROWS) >= 8
    for n in te.BAND16_SMALL_N:
        _assert_same(family, _call(family, row, n=n), _want(family, row, n), "%s %s n = %d" % (family, row, n))


# ---- 3: the routes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", te.FAMILIES)
@pytest.mark.parametrize("row", te.ROUTE_ROWS)
def test_tile_route_equals_forced_general_route(family, row):
    """one band16 row, the window-15 rows L = 28, 36 and 44, and the unbanded call at L = 32 -- the last the tile route serves"""
    assert te.row_kernel(row) != "general"
    tile = _call(family, row)
    general = _call(family, row, general=True)
    _assert_same(family, general, tile, "%s %s general vs tile" % (family, row))
    _assert_same(family, general, _want(family, row), "%s %s general" % (family, row))


@pytest.mark.parametrize("family", te.FAMILIES)
@pytest.mark.parametrize("row", te.GENERAL_ROWS)
def test_windows_past_32_take_the_general_route_with_no_option_set(family, row):
    """an unbanded call at L = 33 and window 33 at L = 110: the rule's results with no option set, and the same with the option"""
    assert te.row_kernel(row) == "general"
    plain = _call(family, row)
    _assert_same(family, plain, _want(family, row), "%s %s" % (family, row))
    _assert_same(family, _call(family, row, general=True), plain, "%s %s forced vs plain" % (family, row))


# ---- 4: the count ---------------------------------------------------------------------------------------------------------------------

def test_count_of_family_row_mode_cases():
    """prints how many (family, row, mode) cases the file holds and how many of them this session ran; a whole run ran them all"""
    cases = te.cases()
    print("tile edge cases (family, row, mode): %d = %d families x %d rows x %d modes; run and right in this session: %d" % (
        len(cases), len(te.FAMILIES), len(te.EDGES), len(te.MODES), len(RAN)))
    assert len(cases) == len(te.FAMILIES) * len(te.EDGES) * len(te.MODES) and RAN <= set(cases)
    assert sorted({(f, r) for f, r, _ in cases}) == EDGE_CASES
