"""MI355X drop-in for ``warpdemux.parallel_distances`` (reference file of the same name).

Same four public functions, argument meanings and error behaviour as the reference
(/root/reference/warpdemux/parallel_distances.py:24-198); the DTW arithmetic runs in the HIP
engine (libwdx_hip.so) instead of dtaidistance's C code.  ``n_jobs`` / ``block_size`` keep their
validation semantics but no process pool is started: one GPU launch covers the whole matrix.

Install in a WarpDemuX process with ``warpdemux_amd.install()``.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _lib


def _as_f64_2d(a, name):
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f"{name} must be 2-dimensional, got shape {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float64)


def _dtw(X: np.ndarray, Y: np.ndarray, window, penalty, want_argmin=False, device=None):
    if X.shape[1] != Y.shape[1]:
        # np.vstack([X, Y]) in the reference raises ValueError on a column mismatch
        raise ValueError(
            f"all the input array dimensions except for the concatenation axis must match exactly, "
            f"but got {X.shape[1]} and {Y.shape[1]} columns"
        )
    ctx = _lib.default_context(device)
    out = np.empty((X.shape[0], Y.shape[0]), dtype=np.float32)
    am = np.empty(X.shape[0], dtype=np.int32) if want_argmin else None
    L = _lib.load()
    _lib.check(
        L.wdx_dtw_matrix(
            ctx.handle, _lib.ptr(X), X.shape[0], _lib.ptr(Y), Y.shape[0], X.shape[1],
            int(window) if window else 0, float(penalty) if penalty else 0.0, _lib.ptr(out), _lib.ptr(am),
        )
    )
    return (out, am) if want_argmin else out


def compute_block_distance(
    block_indices: Tuple[np.ndarray, np.ndarray],
    X,
    window=None,
    penalty=None,
    **kwargs,
):
    """(i, j, float32 block) for the row-index blocks ``i`` x ``j`` of ``X``
    (reference: parallel_distances.py:24-45)."""
    if kwargs:
        raise NotImplementedError(f"unsupported dtaidistance options: {sorted(kwargs)}")
    i, j = block_indices
    X = _as_f64_2d(X, "X")
    return (i, j, _dtw(np.ascontiguousarray(X[i]), np.ascontiguousarray(X[j]), window, penalty))


def distance_matrix_to(
    X,
    Y,
    window: Optional[int] = None,
    penalty: Optional[float] = None,
    block_size: Optional[int] = None,
    n_jobs: int = -1,
    pbar: bool = False,
    pbar_kwargs: dict = {},
):
    """float32 (nX, nY) matrix of banded DTW distances (reference: parallel_distances.py:48-84)."""
    if n_jobs == 1:
        return _dtw(_as_f64_2d(X, "X"), _as_f64_2d(Y, "Y"), window, penalty)
    if block_size is None:
        msg = "block_size must be specified when using parallel."
        logging.error(msg)
        raise ValueError(msg)
    return parallel_distance_matrix_to(
        X, Y, block_size=block_size, n_jobs=n_jobs, window=window, penalty=penalty, pbar=pbar,
        pbar_kwargs=pbar_kwargs,
    )


def parallel_distance_matrix_to(
    X,
    Y,
    block_size: int = 1000,
    n_jobs: int = 6,
    window: Optional[int] = None,
    penalty: Optional[float] = None,
    pbar: bool = False,
    pbar_kwargs: dict = {},
    **kwargs,
):
    """Reference: parallel_distances.py:87-136 (stack X over Y, then the subset form)."""
    X = _as_f64_2d(X, "X")
    Y = _as_f64_2d(Y, "Y")
    if X.shape[1] != Y.shape[1]:
        raise ValueError("X and Y must have the same number of columns")
    return parallel_distance_matrix(
        np.vstack([X, Y]),
        block_size=block_size,
        n_jobs=n_jobs,
        subset=((0, X.shape[0]), (X.shape[0], X.shape[0] + Y.shape[0])),
        window=window,
        penalty=penalty,
        pbar=pbar,
        pbar_kwargs=pbar_kwargs,
        **kwargs,
    )


def parallel_distance_matrix(
    X,
    block_size: int = 1000,
    n_jobs: int = 6,
    subset: Optional[Tuple[Tuple[int, int], Tuple[int, int]]] = None,
    window: Optional[int] = None,
    penalty: Optional[float] = None,
    pbar: bool = False,
    pbar_kwargs: dict = {},
    **kwargs,
):
    """Rows r1 x rows r2 of ``X`` (all-vs-all when ``subset`` is None), float32
    (reference: parallel_distances.py:139-198).  The reference tiles the index space into
    ``block_size`` blocks for its process pool; every block is a full rectangle there
    (``only_triu`` never bites because block columns are offset past the rows), so one launch over
    the whole rectangle returns the same matrix."""
    if kwargs:
        raise NotImplementedError(f"unsupported dtaidistance options: {sorted(kwargs)}")
    X = _as_f64_2d(X, "X")
    if subset:
        (r1_start, r1_end), (r2_start, r2_end) = subset
    else:
        r1_start, r1_end, r2_start, r2_end = 0, X.shape[0], 0, X.shape[0]
    if block_size is None or block_size <= 0:
        raise ValueError("block_size must be a positive integer")
    A = np.ascontiguousarray(X[r1_start:r1_end])
    B = np.ascontiguousarray(X[r2_start:r2_end])
    if pbar:
        from tqdm import tqdm

        with tqdm(total=1, desc="Computing Kernel Matrix", **(pbar_kwargs or {})) as bar:
            out = _dtw(A, B, window, penalty)
            bar.update(1)
        return out
    return _dtw(A, B, window, penalty)


def nearest_reference(X, Y, window=None, penalty=None, wide_dtw=None):
    """(float32 distances (nX,nY), int32 argmin per read) -- SURVEY.md §8 row B3.  ``wide_dtw``: True / False sets
    WDX_OPT_WIDE_DTW on the default context for this call (effective windows 33 .. L on the wide-window kernel); None leaves
    the context as its owner set it.  The reference-named functions above keep the reference's signatures: their users set
    ``_lib.default_context().set_option(_lib.OPT_WIDE_DTW, 1)``."""
    X, Y = _as_f64_2d(X, "X"), _as_f64_2d(Y, "Y")
    if wide_dtw is None:
        return _dtw(X, Y, window, penalty, want_argmin=True)
    if not isinstance(wide_dtw, (bool, np.bool_)):
        raise ValueError(f"nearest_reference: wide_dtw is True, False or None, not {wide_dtw!r}")
    with _lib.default_context().wide_dtw_for_call(bool(wide_dtw)):
        return _dtw(X, Y, window, penalty, want_argmin=True)


def nearest_label(X, Y, labels=None, window=None, penalty=None, min_margin=None, max_dist=None, want_dist=False, n_labels=None):
    """(call int32 (nX,), best float32 (nX, 2) = d1, d2[, float32 distances (nX, nY)]): the nearest reference's label, the
    distance to it and to the nearest reference of another label, and the per-label rejection thresholds -- the rule of
    include/wdx.h (wdx_nearest_dev), the engine's own: the reference ends its classifiers in ``process_probs`` and has no
    function for distances.  ``labels``: one integer label per row of ``Y`` (several references may share one), None for
    the identity; ``min_margin`` / ``max_dist``: a scalar or one float32 threshold per label -- a read is called -1 unless
    ``d2 - d1 >= min_margin[label]`` and ``d1 <= max_dist[label]``.  Without ``want_dist`` the (nX, nY) matrix is not
    returned and, on large batches, never written.  Goes through wdx_set_refs + wdx_dtw_nearest."""
    from . import _nearest

    X, Y = _as_f64_2d(X, "X"), _as_f64_2d(Y, "Y")
    if X.shape[1] != Y.shape[1]:
        raise ValueError(f"X and Y must have the same number of columns, got {X.shape[1]} and {Y.shape[1]}")
    lab, G = _nearest.host_labels(Y.shape[0], labels, n_labels)
    mm = _nearest.host_threshold("min_margin", min_margin, G)
    md = _nearest.host_threshold("max_dist", max_dist, G)
    ctx = _lib.default_context()
    L = _lib.load()
    _lib.check(L.wdx_set_refs(ctx.handle, _lib.ptr(Y), Y.shape[0], Y.shape[1], int(window) if window else 0,
                              float(penalty) if penalty else 0.0))
    n = X.shape[0]
    call = np.empty(n, dtype=np.int32)
    best = np.empty((n, 2), dtype=np.float32)
    dist = np.empty((n, Y.shape[0]), dtype=np.float32) if want_dist else None
    _lib.check(L.wdx_dtw_nearest(ctx.handle, _lib.ptr(X), n, _lib.ptr(lab), G, _lib.ptr(mm), _lib.ptr(md), _lib.ptr(dist),
                                 _lib.ptr(call), _lib.ptr(best)))
    return (call, best, dist) if want_dist else (call, best)


def label_medoids(X, labels, n_labels=None, window=None, penalty=None, status=None, want_cost=False):
    """(index int64 (G,), refs float64 (G, L), count int64 (G,), medoid_cost float64 (G,)[, cost float64 (n,)]): the medoid of
    every label -- the row whose summed DTW distance to the rows of its label is smallest -- as reference signals for
    `nearest_label` / ``wdx_set_refs``.  The rule of include/wdx.h (wdx_medoids_device), the engine's own: the reference ships no
    reference signals and has no code that makes them.  ``labels``: one integer per row of ``X`` in 0 .. G-1, or -1 for a row
    that takes no part; ``status`` (optional): a row whose status is not 0 is no member of its label, like a row with a sample
    that is not finite.  A label without a member has index -1, a NaN cost and a NaN row; ``cost`` of a non-member is NaN.
    A label of more than ``_lib.MEDOID_MAX_GROUP`` rows is NotImplementedError.  Goes through wdx_dtw_medoids; the resident
    reference set is not touched."""
    from . import _medoids

    X = _as_f64_2d(X, "X")
    n, L = X.shape
    lab, G = _medoids.host_labels(n, labels, n_labels)
    st = _medoids.host_status(n, status)
    if L < 1:
        raise ValueError("X must have at least one column")
    index = np.empty(G, dtype=np.int64)
    refs = np.empty((G, L), dtype=np.float64)
    count = np.empty(G, dtype=np.int64)
    mcost = np.empty(G, dtype=np.float64)
    cost = np.empty(n, dtype=np.float64) if want_cost else None
    ctx = _lib.default_context()
    _lib.check(_lib.load().wdx_dtw_medoids(ctx.handle, _lib.ptr(X), n, L, _lib.ptr(lab), G, _lib.ptr(st),
                                           int(window) if window else 0, float(penalty) if penalty else 0.0, _lib.ptr(index),
                                           _lib.ptr(mcost), _lib.ptr(count), _lib.ptr(cost), _lib.ptr(refs)))
    return (index, refs, count, mcost, cost) if want_cost else (index, refs, count, mcost)


def self_distance_matrix(X, window=None, penalty=None, status=None):
    """float32 (n, n): the banded DTW distances of the rows of ``X`` against themselves -- the training matrix of a DTW kernel
    machine (`models.DTW_SVM.fit`) -- with each unordered pair computed once.  The rule of include/wdx.h
    (wdx_self_matrix_device): an entry whose row and column are both members is the float32 `distance_matrix_to(X, X)` holds
    there, bit for bit; a row with a sample that is not finite, or whose ``status`` (optional, one integer per row) is not 0, is
    no member, and its row and column are NaN.  More than ``_lib.SELF_MATRIX_MAX_ROWS`` rows are NotImplementedError.  Goes
    through wdx_dtw_self_matrix; the resident reference set is not touched."""
    from . import _medoids

    X = _as_f64_2d(X, "X")
    n, L = X.shape
    st = _medoids.host_status(n, status)
    if L < 1:
        raise ValueError("X must have at least one column")
    out = np.empty((n, n), dtype=np.float32)
    ctx = _lib.default_context()
    _lib.check(_lib.load().wdx_dtw_self_matrix(ctx.handle, _lib.ptr(X), n, L, _lib.ptr(st), int(window) if window else 0,
                                               float(penalty) if penalty else 0.0, _lib.ptr(out), n))
    return out


def dba_step(X, labels, centres, n_labels=None, window=None, penalty=None, status=None, want_cost=False, want_runs=False):
    """(new_centres float64 (G, L), count int64 (G,), inertia float64 (G,)[, cost float64 (n,)][, runs int32 (n, L, 2)]): one
    step of DTW barycenter averaging -- every member of a label is aligned to the label's current centre, and each centre point
    becomes the mean of the samples matched to it.  The rule of include/wdx.h (wdx_dba_step_device), the engine's own, bit for
    bit; parity with dtaidistance's DBA unpinned.  ``labels`` and ``status`` as for `label_medoids`; ``centres``: one row per
    label.  A label without a member, or whose centre holds a sample that is not finite, is idle: a NaN row, count 0, NaN
    inertia.  ``inertia`` is the summed squared-cost of the centres GIVEN (``cost``: per row, not rooted; ``runs``: the rows
    lo .. hi of each series matched to every centre point).  Goes through wdx_dtw_dba_step; nothing resident is touched."""
    from . import _medoids

    X = _as_f64_2d(X, "X")
    n, L = X.shape
    if n_labels is None and np.ndim(centres) == 2:   # (one centre per label)
        n_labels = int(np.shape(centres)[0])
    lab, G = _medoids.host_labels(n, labels, n_labels, max_group=False)
    st = _medoids.host_status(n, status)
    L = _medoids.dba_length(L)
    C0 = _medoids.host_centres(centres, G, L)
    new = np.empty((G, L), dtype=np.float64)
    count = np.empty(G, dtype=np.int64)
    inertia = np.empty(G, dtype=np.float64)
    cost = np.empty(n, dtype=np.float64) if want_cost else None
    runs = np.empty((n, L, 2), dtype=np.int32) if want_runs else None
    ctx = _lib.default_context()
    _lib.check(_lib.load().wdx_dtw_dba_step(ctx.handle, _lib.ptr(X), n, L, _lib.ptr(lab), G, _lib.ptr(st), _lib.ptr(C0),
                                            int(window) if window else 0, float(penalty) if penalty else 0.0, _lib.ptr(new),
                                            _lib.ptr(count), _lib.ptr(inertia), _lib.ptr(cost), _lib.ptr(runs)))
    return (new, count, inertia) + ((cost,) if want_cost else ()) + ((runs,) if want_runs else ())


def label_barycenters(X, labels, n_labels=None, window=None, penalty=None, status=None, init=None, n_iter=10):
    """(centres float64 (G, L), count int64 (G,), inertia float64 (steps, G)): barycenter reference signals, one per label, by at
    most ``n_iter`` steps of `dba_step` from ``init`` (None: the ``refs`` of `label_medoids`).  The loop stops early when a step
    returns every centre bit-identical to its input; row k of ``inertia`` is the inertia of the centres step k received.  There
    is no tolerance: the caller reads the history.  The centres go straight into ``wdx_set_refs`` / `nearest_label` /
    ``RefineParams(query=...)`` (a label without a member has a NaN row, as with the medoids).  The engine's own rule; parity
    with dtaidistance's DBA unpinned."""
    from . import _medoids

    X = _as_f64_2d(X, "X")
    n, L = X.shape
    lab, G = _medoids.host_labels(n, labels, n_labels, max_group=init is None)   # (the medoids' cap holds for their start only)
    st = _medoids.host_status(n, status)
    L = _medoids.dba_length(L)
    steps = _medoids.n_iterations(n_iter)
    if init is None:
        C0 = label_medoids(X, lab, G, window, penalty, status=st)[1]
    else:
        C0 = _medoids.host_centres(init, G, L).copy()
    hist, count = [], np.zeros(G, dtype=np.int64)
    for _ in range(steps):
        new, count, inertia = dba_step(X, lab, C0, G, window, penalty, status=st)
        hist.append(inertia)
        same = np.array_equal(new.view(np.uint64), C0.view(np.uint64))
        C0 = new
        if same:
            break
    return C0, count, np.array(hist, dtype=np.float64).reshape(len(hist), G)


def _loo_labels(n, labels):
    """int32 labels (n,) or None: an integer dtype, one label per row, none below -1 (-1: the row takes no part)"""
    if labels is None:
        return None
    labels = np.asarray(labels)
    if labels.dtype.kind not in "iu":
        raise ValueError(f"labels must have an integer dtype, not {labels.dtype}")
    if labels.shape != (int(n),):
        raise ValueError(f"labels must hold one label per row: shape ({int(n)},), not {labels.shape}")
    if labels.size and int(labels.min()) < -1:
        raise ValueError(f"labels must be -1 (the row takes no part) or a label >= 0, not {int(labels.min())}")
    if labels.size and int(labels.max()) > np.iinfo(np.int32).max:
        raise ValueError(f"labels must fit an int32, not {int(labels.max())}")
    return np.ascontiguousarray(labels, dtype=np.int32)


def loo_nearest(X, labels=None, window=None, penalty=None, status=None):
    """(nn int32 (n, 2), best float32 (n, 2)): per row of ``X`` the nearest OTHER row of its own label (column 0) and the nearest
    row of any other label (column 1), and the banded DTW distances to them -- what tells whether a labelled set is any good
    before a model is fitted on it (`loo_summary`, `loo_grid`).  The rule of include/wdx.h (wdx_self_nearest_device), the
    engine's own: ``labels`` one integer per row (-1: the row takes no part; None: every row has label 0); a row with a sample
    that is not finite, or whose ``status`` (optional, one integer per row) is not 0, is no member: nn -1, best NaN.  Among
    equal distances the lowest row index wins; a side without a candidate has nn -1 and best +inf.  The distances are those of
    `self_distance_matrix`, bit for bit, but no (n, n) matrix is written: the device memory is O(n L).  More than
    ``_lib.SELF_MATRIX_MAX_ROWS`` rows are NotImplementedError.  Goes through wdx_dtw_self_nearest; nothing resident is touched."""
    from . import _medoids

    X = _as_f64_2d(X, "X")
    n, L = X.shape
    if L < 1:
        raise ValueError("X must have at least one column")
    lab = _loo_labels(n, labels)
    st = _medoids.host_status(n, status)
    if n > _lib.SELF_MATRIX_MAX_ROWS:
        raise NotImplementedError(f"self nearest: n = {n} rows, more than WDX_SELF_MATRIX_MAX_ROWS = {_lib.SELF_MATRIX_MAX_ROWS}: "
                                  "subsample them")
    nn = np.empty((n, 2), dtype=np.int32)
    best = np.empty((n, 2), dtype=np.float32)
    ctx = _lib.default_context()
    _lib.check(_lib.load().wdx_dtw_self_nearest(ctx.handle, _lib.ptr(X), n, L, _lib.ptr(lab), _lib.ptr(st), int(window) if window else 0,
                                                float(penalty) if penalty else 0.0, _lib.ptr(nn), _lib.ptr(best)))
    return nn, best


@dataclass
class LooSummary:
    call: np.ndarray        # int32 (n,)  label of the nearer of the two sides; -1 for a non-member and without any candidate
    margin: np.ndarray      # float32 (n,)  best[:, 1] - best[:, 0]: negative where another label is nearer; NaN for inf - inf and non-members
    confusion: np.ndarray   # int64 (G, G + 1)  members by true label and call; the last column counts call -1
    error_rate: float       # members with a candidate whose call is not their label / members with a candidate (NaN without one)
    n_members: int
    suspects: np.ndarray    # int64: the member rows whose call differs from their label, rising


def loo_summary(labels, nn, best, n_labels=None):
    """`LooSummary` of a `loo_nearest` result, on the host: the leave-one-out 1-nearest-neighbour call of every member (the
    label of the nearer side; on equal distances the lower row index decides), its margin, the confusion of true label by call,
    the error rate and the rows to look at first -- members whose nearest neighbour has another label."""
    nn, best = np.asarray(nn), np.asarray(best)
    if nn.ndim != 2 or nn.shape[1] != 2 or nn.dtype.kind not in "iu":
        raise ValueError(f"nn must be an integer (n, 2) array, not {nn.dtype} {nn.shape}")
    n = nn.shape[0]
    if best.shape != (n, 2) or best.dtype != np.float32:
        raise ValueError(f"best must be a float32 ({n}, 2) array, not {best.dtype} {best.shape}")
    lab = _loo_labels(n, np.zeros(n, dtype=np.int32) if labels is None else labels)
    if n_labels is None:
        G = max(1, int(lab.max()) + 1) if n else 1
    elif isinstance(n_labels, (bool, np.bool_)) or not isinstance(n_labels, (int, np.integer)) or int(n_labels) < 1:
        raise ValueError(f"n_labels must be an integer of at least 1, not {n_labels!r}")
    else:
        G = int(n_labels)
    if n and int(lab.max()) >= G:
        raise ValueError(f"labels must lie in -1 .. {G - 1}")
    if n and (int(nn.min()) < -1 or int(nn.max()) >= n):
        raise ValueError(f"nn must hold row numbers in -1 .. {n - 1}")
    member = (lab >= 0) & ~np.isnan(best[:, 0])
    own, other = nn[:, 0].astype(np.int64), nn[:, 1].astype(np.int64)
    has_own, has_other = member & (own >= 0), member & (other >= 0)
    d_own, d_other = best[:, 0], best[:, 1]
    take_other = has_other & (~has_own | (d_other < d_own) | ((d_other == d_own) & (other < own)))
    call = np.full(n, -1, dtype=np.int32)
    call[has_own] = lab[has_own]
    call[take_other] = lab[other[take_other]]
    with np.errstate(invalid="ignore"):
        margin = (d_other - d_own).astype(np.float32)
    margin[~member] = np.nan
    confusion = np.zeros((G, G + 1), dtype=np.int64)
    np.add.at(confusion, (lab[member], np.where(call[member] < 0, G, call[member])), 1)
    judged = has_own | has_other
    wrong = judged & (call != lab)
    return LooSummary(call=call, margin=margin, confusion=confusion,
                      error_rate=float(wrong.sum()) / float(judged.sum()) if judged.any() else float("nan"),
                      n_members=int(member.sum()), suspects=np.flatnonzero(member & (call != lab)).astype(np.int64))


def loo_grid(X, labels, windows, penalties, status=None):
    """float64 (len(windows), len(penalties)): the leave-one-out 1-nearest-neighbour error rate of the labelled set for every
    window and penalty -- one `loo_nearest` and one `loo_summary` per cell.  The cell with the smallest error is the first
    choice for a chemistry or barcode set the shipped 15 / 0.1 were not chosen for."""
    windows, penalties = list(windows), list(penalties)
    out = np.empty((len(windows), len(penalties)), dtype=np.float64)
    for i, w in enumerate(windows):
        for j, p in enumerate(penalties):
            nn, best = loo_nearest(X, labels, w, p, status=status)
            out[i, j] = loo_summary(labels, nn, best).error_rate
    return out
