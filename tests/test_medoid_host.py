"""The per-label medoid rule (include/wdx.h: wdx_medoids_device) without a GPU: tests/helpers/medoid_rule.py -- the rule in NumPy on the
oracle's float32 dtw_matrix, which the GPU tests compare the device with -- against a brute-force Python loop on tiny inputs; the
refusals of the Python layer that need no device; the constants and symbols of the binding against the header."""
import math
import os
import re

import numpy as np
import pytest

from helpers import medoid_rule as mr
from oracle import wdx_oracle as orc
from warpdemux_amd import _lib, _medoids, parallel_distances as pdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(X, labels, G, window, penalty, status=None):
    """the rule, one pair and one addition at a time"""
    n, L = X.shape
    f = lambda a, b: float(orc.dtw_matrix(X[a:a + 1], X[b:b + 1], window, penalty)[0, 0])   # a float32 value, widened exactly
    member = [labels[r] >= 0 and all(math.isfinite(v) for v in X[r]) and (status is None or status[r] == 0) for r in range(n)]
    cost = [float("nan")] * n
    index, count, mcost = [-1] * G, [0] * G, [float("nan")] * G
    for g in range(G):
        q = [r for r in range(n) if labels[r] == g]
        for r in q:
            if not member[r]:
                continue
            total = 0.0
            for c0 in range(0, len(q), 64):
                s = 0.0
                for j in q[c0:c0 + 64]:
                    if member[j]:
                        s += f(r, j)
                total += s
            cost[r] = total
            count[g] += 1
            if index[g] < 0 or total < mcost[g]:
                index[g], mcost[g] = r, total
    return index, count, mcost, cost


@pytest.mark.parametrize("L, window, penalty", [(7, 2, 0.0), (12, None, 1.5), (25, 15, 0.1)])
def test_helper_is_the_rule_on_tiny_inputs(L, window, penalty):
    rng = np.random.default_rng(L)
    sizes = (1, 2, 70, 0, 5)
    lab = np.concatenate([np.full(m, g) for g, m in enumerate(sizes)] + [np.full(3, -1)]).astype(np.int32)
    rng.shuffle(lab)
    n, G = lab.size, len(sizes)
    X = np.round(rng.normal(0, 1, (n, L)), 1)             # quantised: equal distances and equal costs do occur
    q2 = np.flatnonzero(lab == 2)
    X[q2[3]] = X[q2[1]]                                    # a duplicate row
    X[q2[9], 0] = np.nan
    X[q2[66], L - 1] = -np.inf
    status = np.zeros(n, dtype=np.int32)
    status[q2[30]] = 3
    status[np.flatnonzero(lab == 0)[0]] = 1                # label 0 loses its only row
    got = mr.medoid_rule(X, lab, G, window, penalty, status)
    index, count, mcost, cost = _brute(X, lab, G, window, penalty, status)
    assert got["index"].tolist() == index and got["count"].tolist() == count
    assert mr.same_bits(got["cost"], np.where(np.isnan(cost), mr.QNAN, np.array(cost)))
    assert mr.same_bits(got["medoid_cost"], np.where(np.isnan(mcost), mr.QNAN, np.array(mcost)))
    assert index[0] == -1 and index[3] == -1 and count[2] == 67 and np.isnan(got["refs"][3]).all()
    for g in range(G):
        if index[g] >= 0:
            assert mr.same_bits(got["refs"][g], X[index[g]])
    # more than one chunk was summed, and the chunking matters to the bits somewhere or not -- the totals are the brute force's either way
    assert len(q2) > 64


def test_oracle_distances_are_symmetric_with_a_zero_diagonal():
    """what lets the device take each unordered pair once: f(a, b) == f(b, a) bit for bit on the oracle"""
    rng = np.random.default_rng(5)
    for L, window, penalty in ((7, 2, 0.0), (25, 15, 0.1), (40, 3, 1.5), (110, 15, 0.1), (33, None, 0.7)):
        X = np.round(rng.normal(0, 1, (24, L)), 2)
        X[5] = X[4]
        D = orc.dtw_matrix(X, X, window, penalty)
        assert mr.same_bits(D, np.ascontiguousarray(D.T)) and (np.diag(D) == 0).all()


def test_label_and_status_checks_need_no_device():
    ok = np.array([0, 1, -1, 1], dtype=np.int64)
    lab, G = _medoids.host_labels(4, ok, None)
    assert lab.dtype == np.int32 and lab.tolist() == [0, 1, -1, 1] and G == 2
    assert _medoids.host_labels(0, np.empty(0, dtype=np.int32), None)[1] == 1
    assert _medoids.host_labels(3, np.full(3, -1), None)[1] == 1
    assert _medoids.host_labels(4, ok, 5)[1] == 5
    with pytest.raises(ValueError, match="integer dtype"):
        _medoids.host_labels(4, ok.astype(np.float64), None)
    with pytest.raises(ValueError, match=r"shape \(4,\)"):
        _medoids.host_labels(4, ok[:3], None)
    with pytest.raises(ValueError, match=r"shape \(4,\)"):
        _medoids.host_labels(4, ok.reshape(2, 2), None)
    with pytest.raises(ValueError, match="lie in -1 .. 0"):
        _medoids.host_labels(4, ok, 1)
    with pytest.raises(ValueError, match="lie in -1 .. 1"):
        _medoids.host_labels(4, np.array([0, 1, -2, 1]), 2)
    with pytest.raises(ValueError, match="at least 1"):
        _medoids.host_labels(4, ok, 0)
    with pytest.raises(ValueError, match="n_labels must be an integer"):
        _medoids.host_labels(4, ok, 2.0)
    with pytest.raises(NotImplementedError, match=r"label 1 has 32769 rows.*WDX_MEDOID_MAX_GROUP = 32768"):
        _medoids.host_labels(32772, np.r_[np.zeros(3, dtype=np.int32), np.ones(32769, dtype=np.int32)], None)
    assert _medoids.host_labels(32768, np.zeros(32768, dtype=np.int32), None)[1] == 1      # the cap itself is served
    assert _medoids.host_status(3, None) is None and _medoids.host_status(3, [0, 1, 0]).dtype == np.int32
    with pytest.raises(ValueError, match="status must have an integer dtype"):
        _medoids.host_status(3, [0.0, 1.0, 0.0])
    with pytest.raises(ValueError, match=r"status must hold one value per row"):
        _medoids.host_status(3, [0, 1])


def test_label_medoids_refuses_before_it_reaches_the_library():
    X = np.zeros((4, 25))
    with pytest.raises(ValueError, match="2-dimensional"):
        pdist.label_medoids(np.zeros(25), [0])
    with pytest.raises(ValueError, match="one label per row"):
        pdist.label_medoids(X, [0, 0, 0])
    with pytest.raises(ValueError, match="lie in -1 .. 1"):
        pdist.label_medoids(X, [0, 1, 2, 0], n_labels=2)
    with pytest.raises(ValueError, match="status must hold one value per row"):
        pdist.label_medoids(X, [0, 0, 0, 0], status=[0])


def test_binding_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "wdx.h")).read()
    define = lambda name: int(re.search(r"^#define\s+%s\s+(\d+)" % name, hdr, flags=re.M).group(1))
    assert define("WDX_MEDOID_MAX_GROUP") == 32768 == _lib.MEDOID_MAX_GROUP
    assert define("WDX_OPT_MEDOID_GENERAL") == _lib.OPT_MEDOID_GENERAL and define("WDX_K_MEDOID") == _lib.K_MEDOID
    assert define("WDX_ABI_VERSION") == 4 == _lib.ABI_VERSION      # additions only: the version stays
    L = _lib.load()
    for name in ("wdx_medoids_device", "wdx_dtw_medoids"):
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\(" % name, hdr), name
    assert L.wdx_abi_version() == 4
