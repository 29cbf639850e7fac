"""The edge table of the tile-pass DTW kernels without a GPU (tests/helpers/tile_edges.py): the table reaches every kernel and every
joint of the window-15 row schedule, the two statements of the kernel rule agree, the inputs hold the small magnitudes they were
built to hold (checked with the oracle), and tests/test_gpu_tile_edges.py can run every row of the table: it skips none."""
import functools
import os
import re
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

# (L, window, penalty) of the rows whose inputs go to the oracle: one band16 row at each length and one window-15 row
ORACLE_ROWS = ("b16_40_12", "b16_110_16", "w15_L29")
F32_MIN_NORMAL = np.float32(2.0 ** -126)


def _windows(kernel):
    return sorted({te.effective_window(L, w) for name, (L, w, _) in te.EDGES.items() if te.row_kernel(name) == kernel})


# ---- 1: the table ----------------------------------------------------------------------------------------------------------------

def test_the_table_holds_every_row_the_kernels_were_found_to_need():
    rows = set(te.EDGES.values())
    want = [(L, 15, 0.1) for L in (15, 16, 26, 27, 25, 28, 29, 35, 36, 37, 44, 45)] + [(110, 15, 0.0)]
    want += [(40, 9, 0.1), (40, 12, 0.1), (40, 14, 0.1), (40, 16, 0.1), (110, 16, 0.1), (33, 16, 0.0), (12, 15, 0.1), (16, None, 0.1)]
    want += [(40, 1, 0.1), (40, 8, 0.1), (5, 15, 0.1), (1, None, 0.1), (2, None, 0.1), (8, None, 0.1), (40, 3, 0.0)]
    want += [(110, 17, 0.1), (110, 24, 0.1), (110, 31, 0.1), (40, 20, 0.1), (17, None, 0.1), (32, None, 0.1), (70, 32, 0.0)]
    want += [(33, None, 0.1), (110, 33, 0.1)]
    assert not [r for r in want if r not in rows]
    # L = 25 twice: the short kernel, and the band-15 kernel under WDX_OPT_NO_SHORT_DTW
    assert sorted(n for n, r in te.EDGES.items() if r == (25, 15, 0.1)) == ["w15_L25_no_short", "w15_L25_short"]
    assert te.NO_SHORT == {"w15_L25_no_short"} and te.row_kernel("w15_L25_short") == "short" and te.row_kernel("w15_L25_no_short") == "band15"
    assert all(L <= 110 for L, _, _ in rows)


def test_every_kernel_is_reached_and_each_inexact_one_at_both_ends_of_its_windows():
    assert {te.row_kernel(n) for n in te.EDGES} == {"short", "band8", "band15", "band16", "band32", "general"}
    for kernel, lo, hi in (("band8", 1, 8), ("band16", 9, 16), ("band32", 17, 32)):
        w = _windows(kernel)
        assert w[0] == lo and w[-1] == hi and any(lo < x < hi for x in w), (kernel, w)
        assert 15 not in w
    assert _windows("band15") == [15] and _windows("short") == [15] and min(_windows("general")) == 33
    for name in te.GENERAL_ROWS:
        assert te.row_kernel(name) == "general"
    # the hand-over between the routes: an unbanded call at L = 32 is the last on the tile route, at L = 33 the first off it
    assert te.kernel_of(32, None) == "band32" and te.kernel_of(33, None) == "general" and te.kernel_of(110, 32) == "band32"
    assert all(te.row_kernel(n) != "general" for n in te.ROUTE_ROWS) and "b32_32_unbanded" in te.ROUTE_ROWS
    assert sum(te.row_kernel(n) == "band16" for n in te.ROUTE_ROWS) == 1
    assert {te.EDGES[n][0] for n in te.ROUTE_ROWS if te.row_kernel(n) == "band15"} == {28, 36, 44}


def test_every_joint_of_the_window_15_schedule_is_reached():
    w15 = {n: te.schedule_of(te.EDGES[n][0]) for n in te.EDGES if te.row_kernel(n) == "band15"}
    got = set(w15.values())
    by_L = {te.EDGES[n][0]: s for n, s in w15.items()}
    print(sorted(by_L.items()))
    assert by_L[15] == ("masked", 14, 0, 1) and by_L[27] == ("masked", 14, 0, 13) and by_L[25] == ("masked", 14, 0, 11)
    assert by_L[16] == ("masked", 14, 0, 2) and by_L[26] == ("masked", 14, 0, 12)
    for want in [("pieces", 0, 0, 0), ("pieces", 0, 1, 0), ("pieces", 0, 7, 0), ("pieces", 1, 0, 0), ("pieces", 1, 1, 0), ("pieces", 1, 7, 0),
                 ("pieces", 2, 0, 1), ("pieces", 2, 1, 1), ("pieces", 3, 0, 2)]:
        assert want in got, want
    assert by_L[28] == ("pieces", 0, 0, 0) and by_L[36] == ("pieces", 1, 0, 0) and by_L[44] == ("pieces", 2, 0, 1)
    assert by_L[110] == ("pieces", 10, 2, 9) and any(s[0] == "pieces" and s[1] >= 3 and s[2] > 0 for s in got)
    # the rows that mutation (c) of the summary splits: a remainder behind at least one chunk | no remainder
    assert sorted(L for L, s in by_L.items() if s[0] == "pieces" and s[1] > 0 and s[2] > 0) == [37, 43, 45, 110]
    assert sorted(L for L, s in by_L.items() if s[0] == "pieces" and s[2] == 0) == [28, 36, 44, 52]


def test_schedule_of_restates_the_loops():
    """the closed form against a walk of medoid_band_cost's loops, L = 1 .. 130"""
    W, CH = 15, 8
    for L in range(1, 131):
        if L < 2 * (W - 1):
            i, rows = 0, []
            head_end = min(W - 1, L)
            body_end = max(head_end, L - W + 1)
            for end in (head_end, body_end, L):
                rows.append(end - i)
                i = end
            assert te.schedule_of(L) == ("masked",) + tuple(rows) and sum(rows) == L
            continue
        i, body_end, chunks, prefetches = W - 1, L - W + 1, 0, 0
        while i + CH <= body_end:
            prefetches += i + 2 * CH <= body_end
            chunks += 1
            i += CH
        assert te.schedule_of(L) == ("pieces", chunks, body_end - i, prefetches) and (W - 1) + chunks * CH + (body_end - i) + (W - 1) == L


def test_kernel_of_agrees_with_the_dispatch_rule():
    from helpers.dtw_cases import instantiation

    as_dispatch = {"short": ("short", 15, True), "band15": ("band", 15, True), "band8": ("band", 8, False), "band16": ("band", 16, False),
                   "band32": ("band", 32, False), "general": ("scratch", 0, False)}
    for name, (L, window, _) in te.EDGES.items():
        assert as_dispatch[te.row_kernel(name)] == instantiation(window, L, short=name not in te.NO_SHORT), name
    for L in range(1, 120):
        for window in [None] + list(range(1, 40)):
            for no_short in (False, True):
                assert as_dispatch[te.kernel_of(L, window, no_short)] == instantiation(window, L, short=not no_short), (L, window, no_short)


# ---- 2: every row has its inputs, and the GPU file skips none -------------------------------------------------------------------

@pytest.mark.parametrize("L", sorted({L for L, _, _ in te.EDGES.values()}))
def test_every_length_of_the_table_has_both_inputs_with_their_small_rows(L):
    X0, labels, status = lr.rows(L)
    X, labels1, status1 = te.loo_input(L)
    assert np.array_equal(labels, labels1) and np.array_equal(status, status1) and X.shape == (200, L)
    den, zero, tiny = te.small_rows(X0, labels, status)
    assert len(den) == 5 and len(zero) == 3 and len(tiny) == 2 and len(set(den) | set(zero) | set(tiny)) == 10
    picked = np.concatenate([den, zero, tiny])
    assert not set(picked.tolist()) & set(te.SPECIAL_ROWS) and lr.members(X, labels, status)[picked].all()
    assert len({r // 64 for r in den}) >= 2 and len(set(labels[den])) == 2
    assert len({r // 64 for r in zero}) >= 2 and len(set(labels[zero])) == 2 and tiny.min() > zero[labels[zero] == labels[tiny[0]]].max()
    untouched = np.setdiff1d(np.arange(200), picked)
    assert sr.same_bits(X[untouched], X0[untouched]), "every other row is the generator's own"
    assert sr.same_bits(X[den], X0[den] * 1e-41) and sr.same_bits(X[zero], X0[zero] * 1e-170) and sr.same_bits(X[tiny], X0[tiny] * 1e-150)
    # the special rows keep their roles
    assert np.isnan(X[14, L // 3]) and np.isposinf(X[90, L - 1]) and status[195] == 1 and labels[50] == -1 and labels[120] == 5
    assert all(sr.same_bits(X[r], X[10]) for r in (80, 160, 110, 194)) and np.abs(X[100]).max() > 1e158
    assert int(lr.members(X, labels, status).sum()) == 196
    # the small forms of the band16 rows
    for n in te.BAND16_SMALL_N:
        assert te.loo_input(L, n)[0].shape == (n, L)

    M0, lab, st = mr.labelled_rows(L)[:3]
    M, lab1, st1, G = te.medoid_input(L)
    assert np.array_equal(lab, lab1) and np.array_equal(st, st1) and G == len(mr.SIZES) and M.shape == (531, L)
    den, zero, tiny = te.small_rows(M0, lab, st, avoid=())
    picked = np.concatenate([den, zero, tiny])
    assert len(set(picked.tolist())) == 10 and set(lab[picked]) == {5, 6}, "inside the labels of 129 and 200 rows"
    assert np.isfinite(M[picked]).all() and (st[picked] == 0).all()
    pos = {g: {int(r): k for k, r in enumerate(np.flatnonzero(lab == g))} for g in (5, 6)}   # the medoids' chunks: order within the label
    for rows in (den, zero):
        assert len({(int(lab[r]), pos[int(lab[r])][int(r)] // 64) for r in rows}) >= 3 and len(set(lab[rows])) == 2
    untouched = np.setdiff1d(np.arange(531), picked)
    assert sr.same_bits(M[untouched], M0[untouched])
    assert int(np.isnan(M).any(axis=1).sum()) == 1 and int(np.isinf(M).any(axis=1).sum()) == 1 and int(st.sum()) == 2


def test_the_gpu_file_runs_every_row_for_every_family_and_mode_and_skips_none():
    cases = te.cases()
    assert len(cases) == len(set(cases)) == 3 * len(te.EDGES) * 3 and len(te.EDGES) >= 38
    assert {f for f, _, _ in cases} == {"medoids", "self_matrix", "loo"} and {m for _, _, m in cases} == {0, 1, 2}
    import test_gpu_tile_edges as gpu

    assert gpu.EDGE_CASES == sorted({(f, r) for f, r, _ in cases}) and gpu.te.MODES == (0, 1, 2)
    with open(os.path.join(ROOT, "tests", "test_gpu_tile_edges.py")) as f:
        text = f.read()
    assert not re.search(r"skip|xfail", text), "the GPU file has no way to leave a row out"


# ---- 3: what the inputs hold (the oracle) ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_loo(name):
    L, window, penalty = te.EDGES[name]
    X, labels, status = te.loo_input(L)
    D = sr.self_matrix_rule(X, window, penalty, status)
    mem = lr.members(X, labels, status)
    return D, mem, lr.rule_on_matrix(D, labels, mem)


def _assert_small_blocks(D, den, zero_and_tiny, what):
    """D: the float32 matrix of some rows against themselves (row order: den, then zero_and_tiny)"""
    nd = len(den)
    block = D[:nd, :nd]
    off = block[~np.eye(nd, dtype=bool)]
    assert off.size == nd * (nd - 1) and ((off > 0) & (off < F32_MIN_NORMAL)).all(), (what, off)
    assert (sr.bits(D[nd:, nd:]) == 0).all(), (what, "the zero block is +0.0")
    cross = D[:nd, nd:]
    assert ((cross > 0) & (cross < F32_MIN_NORMAL)).all() and sr.same_bits(cross, np.ascontiguousarray(D[nd:, :nd].T)), what


@pytest.mark.parametrize("name", ORACLE_ROWS)
def test_the_small_rows_give_denormals_and_exact_zeros_on_the_oracle(name):
    from oracle import wdx_oracle as orc

    L, window, penalty = te.EDGES[name]
    assert {te.row_kernel(n) for n in ORACLE_ROWS} == {"band16", "band15"}
    X, labels, status = te.loo_input(L)
    den, zero, tiny = te.small_rows(*lr.rows(L))
    D, mem, (nn, best) = _oracle_loo(name)
    q = np.concatenate([den, zero, tiny])
    _assert_small_blocks(D[np.ix_(q, q)], den, np.concatenate([zero, tiny]), name)
    assert len(den) * (len(den) - 1) == 20
    Dm = D[np.ix_(mem, mem)]
    assert not np.isnan(Dm).any() and not (sr.bits(Dm) >> 31).any(), "no NaN and no sign bit among the members"
    # the leave-one-out expectation: a denormal best on each side, and the zero rows find each other at +0.0
    denormal = (best > 0) & (best < F32_MIN_NORMAL)
    print(name, "denormal best cells", denormal.sum(axis=0).tolist(), "zero best cells", (sr.bits(best) == 0).sum(axis=0).tolist())
    assert denormal[:, 0].any() and denormal[:, 1].any()
    assert denormal[den].all(), "a 1e-41 row's nearest on either side is another one"
    for a, s, b in te.zero_neighbours(labels, zero):
        assert nn[a, s] == b and sr.bits(best)[a, s] == 0, (a, s, b)
    assert len(te.zero_neighbours(labels, zero)) == 5   # A's two rows: each other and B's; B's row: the lower of A's
    # the medoids' input: the same blocks inside the two large labels
    M, lab, st, G = te.medoid_input(L)
    den, zero, tiny = te.small_rows(*mr.labelled_rows(L)[:3], avoid=())
    q = np.concatenate([den, zero, tiny])
    _assert_small_blocks(orc.dtw_matrix(M[q], M[q], window, penalty), den, np.concatenate([zero, tiny]), name + " medoids")
