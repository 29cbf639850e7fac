"""Host code around the device Fpt_Boost trainer (include/wdx.h: wdx_boost_fit_device states the trainer's rule): the borders rule,
the marshalling of one call, and the assembly of the model the resident tail reads.

THE BORDERS RULE (host, once per fit).  Per feature, on the float32 column: ``s`` = the sorted values that are not NaN, ``m`` of them,
``u`` = the unique ones.
- ``len(u) <= 1``: no borders, the feature is never split on;
- ``len(u) - 1 <= B``: the borders are ``u[:-1]``;
- otherwise ``unique(s[(j * m) // (B + 1)] for j = 1 .. B)`` without the values equal to ``u[-1]``.
Borders are ascending float32 data values, and with the tail's ``x > border`` both sides of every border hold a row.
tests/helpers/boost_fit_rule.py restates the whole fit in NumPy."""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional

import numpy as np

from . import _lib


class FitTrees(NamedTuple):
    split_feature: np.ndarray   # int32 (T, depth)
    split_border: np.ndarray    # int32 (T, depth): the index into the feature's borders
    leaf_values: np.ndarray     # float64 (T, 2**depth, k)


def feature_borders(col, border_count: int) -> np.ndarray:
    """The ascending float32 borders of one column (module docstring)."""
    col = np.asarray(col, dtype=np.float32)
    s = np.sort(col[~np.isnan(col)])
    u = np.unique(s)
    if u.size <= 1:
        return np.zeros(0, np.float32)
    if u.size - 1 <= border_count:
        return u[:-1].copy()
    m = s.size
    b = np.unique(s[(np.arange(1, border_count + 1, dtype=np.int64) * m) // (border_count + 1)])
    return b[b != u[-1]]


def borders(X, border_count: int) -> List[np.ndarray]:
    """Per column of ``X`` (n, F) -- float64 rounded to float32 once, as the tail rounds it -- its borders."""
    if not isinstance(border_count, (int, np.integer)) or isinstance(border_count, bool) or border_count < 1:
        raise ValueError(f"border_count must be a positive integer, not {border_count!r}")
    if border_count > _lib.BOOST_FIT_MAX_BORDERS:
        raise NotImplementedError(f"border_count {border_count} (1..{_lib.BOOST_FIT_MAX_BORDERS} supported)")
    with np.errstate(over="ignore"):
        X32 = np.asarray(X, dtype=np.float64).astype(np.float32)
    return [feature_borders(X32[:, f], int(border_count)) for f in range(X32.shape[1])]


def pack_borders(border_list):
    """(the features' borders one after another as float32, n_borders int32) -- what the library reads."""
    bl = [np.asarray(b, dtype=np.float32).ravel() for b in border_list]
    for f, b in enumerate(bl):
        if b.size > 1 and not np.all(b[1:] > b[:-1]):
            raise ValueError(f"the borders of feature {f} must be strictly ascending")
    flat = np.ascontiguousarray(np.concatenate(bl) if bl else np.zeros(0, np.float32), dtype=np.float32)
    if flat.size == 0:
        flat = np.zeros(1, np.float32)   # (a pointer the library may name; it refuses the fit: no feature has a border)
    return flat, np.array([b.size for b in bl], dtype=np.int32)


def params_c(n_features, n_classes, n_trees, depth, border_count, learning_rate, l2_leaf_reg):
    """wdx_boost_fit_params of one call; what Python can name of the plan's refusals is raised here, before any device work."""
    for name, v in (("n_trees", n_trees), ("depth", depth), ("border_count", border_count)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 1:
            raise ValueError(f"{name} must be a positive integer, not {v!r}")
    if depth > _lib.BOOST_FIT_MAX_DEPTH:
        raise NotImplementedError(f"tree depth {depth} (1..{_lib.BOOST_FIT_MAX_DEPTH} supported by the trainer)")
    if border_count > _lib.BOOST_FIT_MAX_BORDERS:
        raise NotImplementedError(f"border_count {border_count} (1..{_lib.BOOST_FIT_MAX_BORDERS} supported)")
    if n_trees > _lib.BOOST_FIT_MAX_TREES:
        raise NotImplementedError(f"{n_trees} trees in one call (1..{_lib.BOOST_FIT_MAX_TREES} supported)")
    if n_classes < 2:
        raise ValueError(f"fit needs at least two classes, found {n_classes}")
    if n_classes > _lib.BOOST_FIT_MAX_CLASSES:
        raise NotImplementedError(f"{n_classes} classes (2..{_lib.BOOST_FIT_MAX_CLASSES} supported)")
    if not 1 <= n_features <= _lib.BOOST_MAX_FEATURES:
        raise NotImplementedError(f"{n_features} features (1..{_lib.BOOST_MAX_FEATURES} supported)")
    if not (np.isscalar(l2_leaf_reg) and np.isreal(l2_leaf_reg) and np.isfinite(l2_leaf_reg) and l2_leaf_reg > 0):
        raise ValueError(f"l2_leaf_reg must be positive and finite, not {l2_leaf_reg!r}")
    if not (np.isscalar(learning_rate) and np.isreal(learning_rate) and np.isfinite(learning_rate)):
        raise ValueError(f"learning_rate must be finite, not {learning_rate!r}")
    p = _lib.BoostFitParamsC()
    p.n_features, p.n_classes, p.n_trees, p.depth, p.border_count = int(n_features), int(n_classes), int(n_trees), int(depth), int(border_count)
    p.reserved = 0
    p.learning_rate, p.l2_leaf_reg = float(learning_rate), float(l2_leaf_reg)
    return p


def call(entry, handle, X_ptr, n, ld, y_ptr, flat, n_borders, p, scores_ptr, stream=None) -> FitTrees:
    """One blocking call of wdx_boost_fit_device (``stream`` given) or wdx_boost_fit: ``p.n_trees`` more trees on the scores."""
    T, D, k = p.n_trees, p.depth, p.n_classes
    sf, sb = np.full((T, D), -1, np.int32), np.full((T, D), -1, np.int32)
    lv = np.full((T, 1 << D, k), np.nan)
    args = [handle, X_ptr, n, ld, y_ptr, _lib.ptr(flat), _lib.ptr(n_borders), C.byref(p), scores_ptr, _lib.ptr(sf), _lib.ptr(sb), _lib.ptr(lv)]
    if stream is not None:
        args.append(stream)
    _lib.check(entry(*args))
    return FitTrees(sf, sb, lv)


def fit_host(X, y_idx, border_list, p, scores, device: Optional[int] = None) -> FitTrees:
    """``p.n_trees`` more trees on HOST arrays through wdx_boost_fit: X (n, F) float64, y_idx (n,) int32, scores (n, k) float64
    C-contiguous, updated in place."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    y_idx = np.ascontiguousarray(y_idx, dtype=np.int32)
    if not (isinstance(scores, np.ndarray) and scores.dtype == np.float64 and scores.flags.c_contiguous and scores.shape == (X.shape[0], p.n_classes)):
        raise ValueError(f"scores must be a C-contiguous float64 ({X.shape[0]}, {p.n_classes}) array")
    flat, nb = pack_borders(border_list)
    ctx = _lib.default_context(device)
    return call(_lib.load().wdx_boost_fit, ctx.handle, _lib.ptr(X), X.shape[0], X.shape[1], _lib.ptr(y_idx), flat, nb, p, _lib.ptr(scores))


def trees_of(fit: FitTrees, border_list):
    """The trees as `models.Fpt_Boost` takes them: (features, float32 border values, nan_true = 0, leaves) per tree."""
    out = []
    for sf, sb, lv in zip(fit.split_feature, fit.split_border, fit.leaf_values):
        out.append((sf.astype(np.int32), np.array([border_list[f][b] for f, b in zip(sf, sb)], dtype=np.float32),
                    np.zeros(len(sf), np.uint8), lv))
    return out
