"""Leave-one-out nearest neighbours without a GPU: the test input holds what it was built to hold (tests/helpers/loo_rule.py:
rows, checked with the oracle on every shape of tests/test_gpu_loo.py), the NumPy rule on injected matrices, and the host side of
the Python layer: `parallel_distances.loo_summary`, `loo_grid` through a stub of `loo_nearest`, and every ValueError the argument
checks raise with no library loaded."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import loo_rule as lr  # noqa: E402
from warpdemux_amd import parallel_distances as pdist  # noqa: E402

# (L, window, penalty) of the GPU test's shapes (the two unbanded ones share their distances)
SHAPES = {"short_25_15": (25, 15, 0.1), "band15_110": (110, 15, 0.1), "band8_40_3": (40, 3, 1.5), "band32_110": (110, 32, 0.1),
          "unbanded_110": (110, None, 0.1)}
INF = np.float32(np.inf)


@functools.lru_cache(maxsize=None)
def _case(shape):
    L, window, penalty = SHAPES[shape]
    X, labels, status = lr.rows(L)
    nn, best = lr.loo_rule(X, labels, window, penalty, status)
    return X, labels, status, nn, best


# ---- 1: the input ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_input_holds_what_it_was_built_to_hold(shape):
    L, window, penalty = SHAPES[shape]
    X, labels, status, nn, best = _case(shape)
    mem = lr.members(X, labels, status)
    assert int(mem.sum()) == 196 and not mem[[14, 90, 195, 50]].any()
    other_nearer = mem & (nn[:, 1] >= 0) & ((nn[:, 0] < 0) | (best[:, 1] < best[:, 0]) | ((best[:, 1] == best[:, 0]) & (nn[:, 1] < nn[:, 0])))
    ties = lr.tie_cells(X, labels, window, penalty, status)
    print(shape, "nearest neighbour of another label:", int(other_nearer.sum()), "tie cells:", ties)
    assert int(other_nearer.sum()) >= 8
    assert ties >= 8
    no_own = np.flatnonzero(mem & (nn[:, 0] < 0))
    assert no_own.tolist() == [120] and best[120, 0] == INF and nn[120, 1] >= 0
    # row 100: every distance to it is +inf, and the lowest candidate index wins on each side
    cand = np.flatnonzero(mem & (np.arange(len(X)) != 100))
    assert best[100, 0] == INF and best[100, 1] == INF
    assert nn[100, 0] == cand[labels[cand] == labels[100]][0] and nn[100, 1] == cand[labels[cand] != labels[100]][0]
    # row 10 and its four copies: exact ties at distance +0 on both sides
    assert nn[10].tolist() == [80, 110] and lr.bits(best[10]).tolist() == [0, 0]
    # the non-members
    for r in (14, 90, 195, 50):
        assert nn[r].tolist() == [-1, -1] and (lr.bits(best[r]) == 0x7FC00000).all()
    # the changed rows span all four chunks
    assert {r // 64 for r in (14, 90, 195, 50, 20, 60, 140, 180, 80, 160, 110, 194, 120, 100)} == {0, 1, 2, 3}


def test_small_inputs_are_left_alone():
    for n in (1, 2, 63, 64, 65, 129):
        X, labels, status = lr.rows(40, n)
        assert X.shape == (n, 40) and np.isfinite(X).all() and (status == 0).all() and labels.min() >= 0 and labels.max() <= 4


# ---- 2: the rule on injected matrices ---------------------------------------------------------------------------------------------

def _inject(D):
    D = np.asarray(D, dtype=np.float32)
    return lambda A, B: D[:len(A), :len(B)].copy()


def test_ties_go_to_the_lowest_index():
    D = np.array([[0, 2, 1, 1, 3, 3],
                  [2, 0, 2, 2, 2, 2],
                  [1, 2, 0, 5, 4, 4],
                  [1, 2, 5, 0, 1, 1],
                  [3, 2, 4, 1, 0, 9],
                  [3, 2, 4, 1, 9, 0]], dtype=np.float32)
    labels = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    nn, best = lr.loo_rule(np.zeros((6, 3)), labels, matrix=_inject(D))
    assert nn.tolist() == [[2, 3], [0, 3], [0, 4], [4, 0], [3, 1], [3, 1]]
    assert best.tolist() == [[1, 1], [2, 2], [1, 4], [1, 1], [1, 2], [1, 2]]


def test_each_row_uses_its_own_entries():
    D = np.array([[0, 1, 7], [5, 0, 2], [3, 9, 0]], dtype=np.float32)   # not symmetric on purpose
    nn, best = lr.loo_rule(np.zeros((3, 2)), np.array([0, 0, 1]), matrix=_inject(D))
    assert nn.tolist() == [[1, 2], [0, 2], [-1, 0]] and best.tolist() == [[1, 7], [5, 2], [np.inf, 3]]


def test_an_all_inf_row_takes_the_first_candidate():
    D = np.full((4, 4), np.inf, dtype=np.float32)
    np.fill_diagonal(D, 0)
    nn, best = lr.loo_rule(np.zeros((4, 2)), np.array([1, 0, 1, 0]), matrix=_inject(D))
    assert nn.tolist() == [[2, 1], [3, 0], [0, 1], [1, 0]] and np.isposinf(best).all()


def test_one_row_and_no_labels():
    nn, best = lr.loo_rule(np.zeros((1, 5)), np.array([3]), matrix=_inject([[0]]))
    assert nn.tolist() == [[-1, -1]] and np.isposinf(best).all()
    D = np.array([[0, 4, 2], [4, 0, 1], [2, 1, 0]], dtype=np.float32)
    nn, best = lr.loo_rule(np.zeros((3, 2)), None, matrix=_inject(D))
    assert nn.tolist() == [[2, -1], [2, -1], [1, -1]] and best.tolist() == [[2, np.inf], [1, np.inf], [1, np.inf]]


def test_non_members_are_left_out_and_get_the_quiet_nan():
    X = np.zeros((4, 2))
    X[1, 0] = np.nan
    D = np.array([[0, 1], [1, 0]], dtype=np.float32)   # the members' matrix: rows 0 and 3
    nn, best = lr.loo_rule(X, np.array([0, 0, -1, 0]), status=np.array([0, 0, 0, 0]), matrix=_inject(D))
    assert nn.tolist() == [[3, -1], [-1, -1], [-1, -1], [0, -1]]
    assert (lr.bits(best[[1, 2]]) == 0x7FC00000).all() and best[0].tolist() == [1, np.inf]


# ---- 3: loo_summary and loo_grid --------------------------------------------------------------------------------------------------

HAND_LABELS = np.array([0, 0, 1, 1, 2, -1, 1, 0], dtype=np.int32)
QN = lr.QNAN32
HAND_NN = np.array([[1, 2], [0, 3], [3, 0], [2, 1], [-1, 0], [-1, -1], [2, 1], [-1, -1]], dtype=np.int32)
HAND_BEST = np.array([[1, 2], [3, 2], [2, 2], [np.inf, np.inf], [np.inf, 4], [QN, QN], [5, 5], [QN, QN]], dtype=np.float32)
# row 0: own nearer -> 0      row 1: other nearer -> 1 (a suspect)      row 2: equal, the other side's row 0 < 3 -> 0 (a suspect)
# row 3: inf == inf, other row 1 < own row 2 -> label 0 (a suspect)      row 4: no own candidate -> label of row 0 (a suspect)
# row 5: label -1; row 7: a non-member with a label (NaN)      row 6: equal at 5, other row 1 < own row 2 -> 0 (a suspect)


def test_loo_summary_on_a_hand_made_case():
    S = pdist.loo_summary(HAND_LABELS, HAND_NN, HAND_BEST)
    assert S.call.dtype == np.int32 and S.call.tolist() == [0, 1, 0, 0, 0, -1, 0, -1]
    assert S.margin.dtype == np.float32
    assert S.margin[[0, 1, 2, 6]].tolist() == [1, -1, 0, 0] and np.isnan(S.margin[[3, 5, 7]]).all() and S.margin[4] == -np.inf
    assert S.n_members == 6 and S.suspects.dtype == np.int64 and S.suspects.tolist() == [1, 2, 3, 4, 6]
    assert S.confusion.dtype == np.int64 and S.confusion.tolist() == [[1, 1, 0, 0], [3, 0, 0, 0], [1, 0, 0, 0]]
    assert S.error_rate == 5 / 6
    wide = pdist.loo_summary(HAND_LABELS, HAND_NN, HAND_BEST, n_labels=4)
    assert wide.confusion.shape == (4, 5) and wide.confusion[:3, :3].tolist() == [[1, 1, 0], [3, 0, 0], [1, 0, 0]] and wide.confusion.sum() == 6


def test_loo_summary_counts_a_member_without_any_candidate_as_minus_one():
    S = pdist.loo_summary(np.array([2]), np.array([[-1, -1]], dtype=np.int32), np.full((1, 2), np.inf, dtype=np.float32))
    assert S.call.tolist() == [-1] and S.n_members == 1 and S.confusion.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]]
    assert np.isnan(S.error_rate) and S.suspects.tolist() == [0] and np.isnan(S.margin[0])
    E = pdist.loo_summary(np.zeros(0, dtype=np.int32), np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2), dtype=np.float32))
    assert E.n_members == 0 and E.confusion.tolist() == [[0, 0]] and np.isnan(E.error_rate)


def test_loo_summary_on_the_rule_of_the_test_input():
    X, labels, status, nn, best = _case("band8_40_3")
    S = pdist.loo_summary(labels, nn, best)
    mem = lr.members(X, labels, status)
    assert S.n_members == 196 and S.confusion.shape == (6, 7) and S.confusion.sum() == 196
    assert (S.call[~mem] == -1).all() and np.isnan(S.margin[~mem]).all()
    assert np.array_equal(S.suspects, np.flatnonzero(mem & (S.call != labels)))
    assert {20, 60, 140, 180, 120}.issubset(set(S.suspects.tolist())), "the mislabelled rows and the lone label are suspects"
    assert S.error_rate == len(S.suspects) / 196 and S.call[10] == labels[10]   # (row 10: 80 < 110)


def test_loo_grid_is_the_loop_over_loo_nearest(monkeypatch):
    calls = []

    def stub(X, labels=None, window=None, penalty=None, status=None):
        calls.append((window, penalty, status))
        best = HAND_BEST.copy()
        if window == 7:            # a better window: rows 1 and 2 come right
            best[1] = (1, 2)
            best[2] = (1, 2)
        if penalty == 0.5:         # ... and a better penalty: row 6 too
            best[6] = (4, 5)
        return HAND_NN.copy(), best

    monkeypatch.setattr(pdist, "loo_nearest", stub)
    E = pdist.loo_grid(np.zeros((8, 3)), HAND_LABELS, [15, 7], [0.1, 0.5, None], status="S")
    assert E.dtype == np.float64 and E.shape == (2, 3)
    assert E.tolist() == [[5 / 6, 4 / 6, 5 / 6], [3 / 6, 2 / 6, 3 / 6]]
    assert calls == [(15, 0.1, "S"), (15, 0.5, "S"), (15, None, "S"), (7, 0.1, "S"), (7, 0.5, "S"), (7, None, "S")]


# ---- 4: the argument checks, with no library loaded ----------------------------------------------------------------------------------

def test_every_value_error_is_raised_before_the_library_is_touched(monkeypatch):
    from warpdemux_amd import _lib

    def no_library(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "default_context", no_library)
    X = np.zeros((4, 3))
    with pytest.raises(ValueError, match="X must be 2-dimensional"):
        pdist.loo_nearest(np.zeros(4))
    with pytest.raises(ValueError, match="X must have at least one column"):
        pdist.loo_nearest(np.zeros((4, 0)))
    with pytest.raises(ValueError, match="labels must have an integer dtype"):
        pdist.loo_nearest(X, np.zeros(4))
    with pytest.raises(ValueError, match=r"labels must hold one label per row: shape \(4,\)"):
        pdist.loo_nearest(X, np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError, match="labels must be -1 .* or a label >= 0, not -2"):
        pdist.loo_nearest(X, np.array([0, 1, -2, 0]))
    with pytest.raises(ValueError, match="status must have an integer dtype"):
        pdist.loo_nearest(X, None, status=np.zeros(4))
    with pytest.raises(ValueError, match=r"status must hold one value per row: shape \(4,\)"):
        pdist.loo_nearest(X, None, status=np.zeros((4, 1), dtype=np.int32))
    with pytest.raises(NotImplementedError, match="n = 65537 rows, more than WDX_SELF_MATRIX_MAX_ROWS = 65536"):
        pdist.loo_nearest(np.zeros((65537, 1)))
    # loo_summary is host only
    with pytest.raises(ValueError, match=r"nn must be an integer \(n, 2\) array"):
        pdist.loo_summary(HAND_LABELS, HAND_NN[:, :1], HAND_BEST)
    with pytest.raises(ValueError, match=r"best must be a float32 \(8, 2\) array"):
        pdist.loo_summary(HAND_LABELS, HAND_NN, HAND_BEST.astype(np.float64))
    with pytest.raises(ValueError, match="labels must hold one label per row"):
        pdist.loo_summary(HAND_LABELS[:5], HAND_NN, HAND_BEST)
    with pytest.raises(ValueError, match=r"labels must lie in -1 \.\. 1"):
        pdist.loo_summary(HAND_LABELS, HAND_NN, HAND_BEST, n_labels=2)
    with pytest.raises(ValueError, match="n_labels must be an integer of at least 1"):
        pdist.loo_summary(HAND_LABELS, HAND_NN, HAND_BEST, n_labels=0)
    with pytest.raises(ValueError, match=r"nn must hold row numbers in -1 \.\. 7"):
        pdist.loo_summary(HAND_LABELS, HAND_NN + 7, HAND_BEST)
