"""Accuracy thresholds from probabilities and labels (include/wdx.h: wdx_accuracy_thresholds_device states the rule): the per-class
confidence margins below which ``process_probs`` leaves a read uncalled, chosen so that the calls that remain reach a target
accuracy on labelled probabilities.

The reference ships such tables (``target_accuracy_thresholds/*.csv``) but not the procedure that made them, so THE RULE is this
engine's own and parity with the reference's values is unpinned:

  * a row is used when ``y_idx >= 0`` and all its probabilities are finite (the rest are counted in ``skipped``);
  * ``p`` = the first maximum, ``conf = top1 - top2`` (float64);
  * the grid is ``g_i = i / R`` (one float64 division), ``bin`` = the largest i with ``g_i <= conf``;
  * ``kept[c][j]`` / ``hit[c][j]``: the used rows called c with ``bin >= j``, and those of them with ``y_idx == c``;
  * the threshold of class c for a target of a per mille is ``g_j`` for the smallest ``j >= 1`` with ``kept[c][j] > 0`` and
    ``1000 * hit[c][j] >= a * kept[c][j]`` (integers: exact), ``+inf`` when no j qualifies.

`rule` restates it in NumPy (no device); `host` runs wdx_accuracy_thresholds on host arrays.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib


def targets_per_mille(targets):
    """int32 (T,): each target accuracy, a fraction in 0 .. 1, as a whole number of per mille (``int(round(t * 1000))``).
    ValueError for one that is not."""
    ts = np.atleast_1d(np.asarray(targets, dtype=np.float64))
    if ts.ndim != 1 or not 1 <= ts.size <= _lib.THRESHOLDS_MAX_TARGETS:
        raise ValueError(f"targets must hold 1 .. {_lib.THRESHOLDS_MAX_TARGETS} values")
    out = []
    for t in ts:
        if not np.isfinite(t) or not 0.0 <= t <= 1.0:
            raise ValueError(f"a target accuracy must lie in 0 .. 1, not {t!r}")
        pm = int(round(float(t) * 1000))
        if abs(float(t) * 1000 - pm) > 1e-6:
            raise ValueError(f"a target accuracy must be a whole number of per mille, not {float(t)!r}")
        out.append(pm)
    return np.array(out, dtype=np.int32)


def check_sizes(k, resolution):
    if not 2 <= int(k) <= _lib.THRESHOLDS_MAX_CLASSES:
        raise ValueError(f"k = {k} classes (2..{_lib.THRESHOLDS_MAX_CLASSES})")
    if not 1 <= int(resolution) <= _lib.THRESHOLDS_MAX_RESOLUTION:
        raise ValueError(f"resolution = {resolution} (1..{_lib.THRESHOLDS_MAX_RESOLUTION})")


def rule(prob, y_idx, targets_pm, resolution):
    """(thr float64 (T, k), kept int64 (k, R + 1), hit int64 (k, R + 1), skipped int) by the stated rule, in NumPy."""
    prob = np.asarray(prob, dtype=np.float64)
    y_idx = np.asarray(y_idx)
    n, k = prob.shape
    R = int(resolution)
    check_sizes(k, R)
    targets_pm = np.asarray(targets_pm, dtype=np.int64)
    used = (y_idx >= 0) & np.isfinite(prob).all(axis=1)
    P, y = prob[used], y_idx[used]
    p = np.argmax(P, axis=1) if len(P) else np.zeros(0, np.int64)
    top1 = P[np.arange(len(P)), p]
    rest = P.copy()
    rest[np.arange(len(P)), p] = -np.inf
    with np.errstate(over="ignore"):
        conf = top1 - rest.max(axis=1) if len(P) else np.zeros(0)
    grid = np.arange(R + 1, dtype=np.float64) / np.float64(R)
    bins = np.searchsorted(grid, conf, side="right") - 1          # the largest i with g_i <= conf (conf >= 0 = g_0)
    N = np.zeros((k, R + 1), np.int64)
    H = np.zeros((k, R + 1), np.int64)
    np.add.at(N, (p, bins), 1)
    np.add.at(H, (p[p == y], bins[p == y]), 1)
    kept = np.cumsum(N[:, ::-1], axis=1)[:, ::-1]
    hit = np.cumsum(H[:, ::-1], axis=1)[:, ::-1]
    thr = np.full((len(targets_pm), k), np.inf)
    for t, a in enumerate(targets_pm):
        ok = (kept[:, 1:] > 0) & (1000 * hit[:, 1:] >= int(a) * kept[:, 1:])
        for c in range(k):
            j = np.flatnonzero(ok[c])
            if len(j):
                thr[t, c] = grid[j[0] + 1]
    return thr, np.ascontiguousarray(kept), np.ascontiguousarray(hit), int(n - used.sum())


def host(prob, y_idx, targets_pm, resolution, device: Optional[int] = None):
    """The same on the device through wdx_accuracy_thresholds: host arrays in and out, one synchronisation."""
    prob = np.ascontiguousarray(prob, dtype=np.float64)
    if prob.ndim != 2:
        raise ValueError(f"prob must be (n, k), not {prob.shape}")
    n, k = prob.shape
    y_idx = np.ascontiguousarray(y_idx, dtype=np.int32)
    if y_idx.shape != (n,):
        raise ValueError(f"y_idx must hold one class index per row: shape ({n},), not {y_idx.shape}")
    R = int(resolution)
    check_sizes(k, R)
    targets_pm = np.ascontiguousarray(targets_pm, dtype=np.int32)
    T = len(targets_pm)
    thr = np.empty((T, k))
    kept, hit = np.empty((k, R + 1), np.int64), np.empty((k, R + 1), np.int64)
    skipped = np.zeros(1, np.int64)
    ctx = _lib.default_context(device)
    _lib.check(_lib.load().wdx_accuracy_thresholds(ctx.handle, _lib.ptr(prob), n, k, _lib.ptr(y_idx), R, _lib.ptr(targets_pm), T, _lib.ptr(thr),
                                                   _lib.ptr(kept), _lib.ptr(hit), _lib.ptr(skipped)))
    return thr, kept, hit, int(skipped[0])
