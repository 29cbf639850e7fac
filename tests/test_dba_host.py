"""The barycenter step's rule (include/wdx.h: wdx_dba_step_device) without a GPU: tests/helpers/dba_rule.py -- the rule in NumPy,
which the GPU tests compare the device with -- against the oracle's distances, against a brute force over every monotone band path
on tiny inputs, and over twelve successive steps; the share of tied cells in the input of the GPU tie test; the refusals of the
Python layer that need no device; the constants and symbols of the binding against the header."""
import math
import os
import re

import numpy as np
import pytest

from helpers import dba_rule as dr
from helpers import medoid_rule as mr
from oracle import wdx_oracle as orc
from warpdemux_amd import _lib, _medoids, parallel_distances as pdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(25, 15, 0.1), (110, 15, 0.1), (40, None, 0)]


def _step(L, window, penalty):
    X, lab, status, G = mr.labelled_rows(L)
    Cm = mr.medoid_rule(X, lab, G, window, penalty, status)["refs"]
    return X, lab, G, Cm, dr.dba_step(X, lab, Cm, G, window, penalty, status)


@pytest.mark.parametrize("L,window,penalty", SHAPES)
def test_rooted_cost_is_the_oracles_distance_and_the_runs_chain(L, window, penalty):
    X, lab, G, Cm, r = _step(L, window, penalty)
    assert r["count"].tolist() == [1, 2, 63, 64, 64, 128, 199, 0, 0]
    for g in range(G):
        q = np.flatnonzero((lab == g) & ~np.isnan(r["cost"]))
        assert q.size == r["count"][g]
        if q.size:
            D = orc.dtw_matrix(X[q], Cm[g:g + 1], window, penalty)[:, 0]
            assert mr.same_bits(np.sqrt(r["cost"][q]).astype(np.float32), D), g
    member = ~np.isnan(r["cost"])
    lo, hi = r["runs"][member].transpose(2, 0, 1)
    assert (lo[:, 0] == 0).all() and (hi[:, -1] == L - 1).all() and (lo <= hi).all()
    assert (hi[:, :-1] <= lo[:, 1:]).all() and (lo[:, 1:] <= hi[:, :-1] + 1).all()
    assert (r["runs"][~member] == -1).all() and np.isnan(r["new_centres"][[7, 8]]).all() and np.isnan(r["inertia"][[7, 8]]).all()
    # the centre is the mean of the matched samples, and the inertia the sum of the costs (to rounding; the bits are the GPU tests' matter)
    g = 6
    q = np.flatnonzero((lab == g) & member)
    T, K = np.zeros(L), np.zeros(L)
    for row in q:
        for j in range(L):
            a, b = r["runs"][row, j]
            T[j] += X[row, a:b + 1].sum()
            K[j] += b - a + 1
    assert np.allclose(r["new_centres"][g], T / K, rtol=1e-12, atol=0) and math.isclose(r["inertia"][g], r["cost"][q].sum(), rel_tol=1e-12)


def _band_minimum(x, c, window, p2):
    """the smallest accumulated cost over every monotone path inside the band, each sum taken in the recurrence's own order"""
    L = len(x)
    w = window if window else L
    best = math.inf

    def rec(i, j, acc):
        nonlocal best
        if abs(i - j) > w - 1:
            return
        d = x[i] - c[j]
        acc = d * d + acc
        if i == L - 1 and j == L - 1:
            best = min(best, acc)
            return
        if i + 1 < L and j + 1 < L:
            rec(i + 1, j + 1, acc)
        if i + 1 < L:
            rec(i + 1, j, acc + p2)
        if j + 1 < L:
            rec(i, j + 1, acc + p2)

    rec(0, 0, 0.0)
    return best


@pytest.mark.parametrize("L,window,penalty", [(1, None, 0.3), (2, 1, 0.1), (4, 2, 0.1), (5, 3, 0.0), (6, None, 0.25), (6, 4, 1.5), (6, 6, 0.0)])
def test_the_rules_path_is_a_cheapest_band_path(L, window, penalty):
    rng = np.random.default_rng(L * 31 + (window or 0))
    X = np.concatenate([rng.normal(0, 1, (12, L)), rng.integers(-1, 2, (12, L)).astype(np.float64)])
    c = X[3] + rng.normal(0, 0.3, L) if L > 1 else np.array([0.25])
    p2 = np.float64(penalty) * np.float64(penalty)
    a = dr.align(X, c, window, penalty)
    w = dr.effective_window(L, window)
    for r in range(len(X)):
        cells = sorted((i, j) for j in range(L) for i in range(a["lo"][r, j], a["hi"][r, j] + 1))
        assert cells[0] == (0, 0) and cells[-1] == (L - 1, L - 1) and all(abs(i - j) < w for i, j in cells)
        acc, prev = 0.0, None
        for i, j in cells:
            if prev is not None:
                di, dj = i - prev[0], j - prev[1]
                assert (di, dj) in ((1, 1), (1, 0), (0, 1)), (prev, (i, j))
                if di + dj == 1:
                    acc = acc + p2
            d = X[r, i] - c[j]
            acc = d * d + acc
            prev = (i, j)
        assert acc == a["cost"][r] == _band_minimum(X[r], c, window, p2), (r, acc, a["cost"][r])


def test_twelve_steps_never_raise_a_labels_inertia():
    L, window, penalty = 25, 15, 0.1
    X, lab, status, G = mr.labelled_rows(L)
    init = mr.medoid_rule(X, lab, G, window, penalty, status)["refs"]
    C, count, hist = dr.barycenters(X, lab, init, G, window, penalty, status, n_iter=12)
    busy = [0, 1, 2, 3, 4, 5, 6]
    assert 2 <= len(hist) <= 12 and (np.diff(hist[:, busy], axis=0) <= 0).all(), hist[:, busy]
    assert hist[-1, 6] < 0.95 * hist[0, 6] and np.isnan(hist[:, [7, 8]]).all() and np.isnan(C[[7, 8]]).all()


@pytest.mark.parametrize("penalty", [0, 0.5])
def test_the_tie_input_of_the_gpu_test_ties(penalty):
    """at least a tenth of the path steps of helpers.dba_rule.tied_input(40) at window 8 sit on a cell with equal predecessors"""
    X, lab, Cm, G = dr.tied_input(40)
    for g in range(G):
        share = dr.tied_share(X[lab == g], Cm[g], 8, penalty)
        print("label", g, "penalty", penalty, "tied share %.3f" % share)
        assert share >= 0.1, (g, share)


def test_python_refuses_before_it_reaches_the_library():
    X = np.zeros((4, 25))
    Cm = np.zeros((2, 25))
    with pytest.raises(ValueError, match="2-dimensional"):
        pdist.dba_step(np.zeros(25), [0], Cm)
    with pytest.raises(ValueError, match="one label per row"):
        pdist.dba_step(X, [0, 0, 0], Cm)
    with pytest.raises(ValueError, match="lie in -1 .. 1"):
        pdist.dba_step(X, [0, 1, 2, 0], Cm)
    with pytest.raises(ValueError, match=r"centres must hold one row per label: shape \(3, 25\)"):
        pdist.dba_step(X, [0, 1, 2, 0], Cm, n_labels=3)
    with pytest.raises(ValueError, match="n_labels must be at least 1"):
        pdist.dba_step(X, [-1, -1, -1, -1], Cm, n_labels=0)
    with pytest.raises(ValueError, match="status must hold one value per row"):
        pdist.dba_step(X, [0, 0, 0, 0], Cm, status=[0])
    with pytest.raises(NotImplementedError, match="L = 1025 is more than WDX_DBA_MAX_L = 1024"):
        pdist.dba_step(np.zeros((2, 1025)), [0, 0], np.zeros((1, 1025)))
    with pytest.raises(ValueError, match="n_iter must be an integer of at least 1"):
        pdist.label_barycenters(X, [0, 0, 1, 1], n_iter=0)
    with pytest.raises(ValueError, match="centres must hold one row per label"):
        pdist.label_barycenters(X, [0, 0, 1, 1], init=np.zeros((3, 25)))
    assert _medoids.dba_length(1024) == 1024 and _medoids.host_centres([[1, 2]], 1, 2).dtype == np.float64


def test_binding_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "wdx.h")).read()
    define = lambda name: int(re.search(r"^#define\s+%s\s+(\d+)" % name, hdr, flags=re.M).group(1))
    assert define("WDX_OPT_DBA_GENERAL") == 27 == _lib.OPT_DBA_GENERAL
    assert define("WDX_DBA_MAX_L") == 1024 == _lib.DBA_MAX_L
    assert define("WDX_ABI_VERSION") == 4 == _lib.ABI_VERSION      # additions only: the version stays
    L = _lib.load()
    for name in ("wdx_dba_step_device", "wdx_dtw_dba_step"):
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\(" % name, hdr), name
    assert L.wdx_abi_version() == 4
    assert "parity with dtaidistance" in open(os.path.join(ROOT, "README.md")).read()
