"""NumPy restatements for the tests of the kernel matrix and the accuracy thresholds (include/wdx.h: wdx_svm_kernel_device,
wdx_accuracy_thresholds_device), written from the rules and not from the library's Python.

  kernel_matrix      K = float32(exp_rule(-(gamma * D^p))), every operation float64 and rounded on its own; exp_rule as
                     helpers/boost_fit_rule.py states it
  thresholds_brute   the threshold rule by sorting and counting, row by row and grid value by grid value: no histogram, no
                     suffix sum, no bin formula
"""
from __future__ import annotations

import numpy as np

from . import boost_fit_rule


def kernel_matrix(D, gamma, pwr_dist):
    t = np.asarray(D, dtype=np.float32).astype(np.float64)
    w = t.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(int(pwr_dist) - 1):
            w = w * t
        x = -(np.float64(gamma) * w)
    nan = np.isnan(x)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        e = boost_fit_rule.exp_rule(np.where(nan, 0.0, x))
        out = np.where(nan, x, e).astype(np.float32)
    return out


def thresholds_brute(prob, y_idx, targets_pm, R):
    """(thr (T, k), kept (k, R + 1), hit (k, R + 1), skipped): counts by comparison of every used row's margin with every grid
    value."""
    prob = np.asarray(prob, dtype=np.float64)
    n, k = prob.shape
    grid = [np.float64(i) / np.float64(R) for i in range(R + 1)]
    rows = []
    skipped = 0
    for r in range(n):
        if y_idx[r] < 0 or not all(np.isfinite(v) for v in prob[r]):
            skipped += 1
            continue
        order = sorted(range(k), key=lambda c: (-prob[r, c], c))       # first maximum first
        p = order[0]
        with np.errstate(over="ignore"):
            conf = prob[r, p] - prob[r, order[1]]
        rows.append((p, conf, p == y_idx[r]))
    kept = np.zeros((k, R + 1), np.int64)
    hit = np.zeros((k, R + 1), np.int64)
    for c in range(k):
        confs = np.array([cf for p, cf, _ in rows if p == c], dtype=np.float64)
        right = np.array([ok for p, _, ok in rows if p == c], dtype=bool)
        for j in range(R + 1):
            sel = confs >= grid[j]
            kept[c, j] = int(sel.sum())
            hit[c, j] = int((sel & right).sum())
    thr = np.full((len(targets_pm), k), np.inf)
    for t, a in enumerate(targets_pm):
        for c in range(k):
            for j in range(1, R + 1):
                if kept[c, j] > 0 and 1000 * int(hit[c, j]) >= int(a) * int(kept[c, j]):
                    thr[t, c] = grid[j]
                    break
    return thr, kept, hit, skipped
