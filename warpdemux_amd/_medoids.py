"""Arguments of the per-label medoid rule (include/wdx.h: wdx_medoids_device), checked on the host once for both Python ways in:
`parallel_distances.label_medoids` and `DemuxEngine.medoids`.  Nothing here touches a GPU."""
from __future__ import annotations

import numpy as np

from . import _lib


def host_labels(n, labels, n_labels, max_group=True):
    """(int32 labels (n,), G): an integer dtype, one label per row, every label in -1 .. G-1 (-1: the row takes no part);
    ``n_labels`` None: the largest label + 1 (at least 1).  A label of more than `_lib.MEDOID_MAX_GROUP` rows is
    NotImplementedError: the caller subsamples (``max_group`` False: no such cap -- a barycenter step has none)."""
    labels = np.asarray(labels)
    if labels.dtype.kind not in "iu":
        raise ValueError(f"labels must have an integer dtype, not {labels.dtype}")
    if labels.shape != (int(n),):
        raise ValueError(f"labels must hold one label per row: shape ({int(n)},), not {labels.shape}")
    if n_labels is None:
        G = max(1, int(labels.max()) + 1) if labels.size else 1
    elif isinstance(n_labels, (bool, np.bool_)) or not isinstance(n_labels, (int, np.integer)):
        raise ValueError(f"n_labels must be an integer, not {n_labels!r}")
    else:
        G = int(n_labels)
    if G < 1:
        raise ValueError(f"n_labels must be at least 1, not {G}")
    if labels.size and (int(labels.min()) < -1 or int(labels.max()) >= G):
        raise ValueError(f"labels must lie in -1 .. {G - 1}")
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if labels.size and max_group:
        sizes = np.bincount(labels[labels >= 0], minlength=G)
        g = int(np.argmax(sizes))
        if sizes[g] > _lib.MEDOID_MAX_GROUP:
            raise NotImplementedError(f"medoids: label {g} has {int(sizes[g])} rows, more than WDX_MEDOID_MAX_GROUP = "
                                      f"{_lib.MEDOID_MAX_GROUP}: subsample it")
    return labels, G


def dba_length(L):
    """L of a barycenter step (include/wdx.h: wdx_dba_step_device): 1 .. `_lib.DBA_MAX_L`"""
    if int(L) < 1:
        raise ValueError("X must have at least one column")
    if int(L) > _lib.DBA_MAX_L:
        raise NotImplementedError(f"dba: L = {int(L)} is more than WDX_DBA_MAX_L = {_lib.DBA_MAX_L}")
    return int(L)


def host_centres(centres, G, L):
    """float64 centres (G, L) of a barycenter step on the host: one row per label (a row with a sample that is not finite makes
    its label idle)"""
    centres = np.asarray(centres)
    if centres.ndim != 2 or centres.shape != (int(G), int(L)):
        raise ValueError(f"centres must hold one row per label: shape ({int(G)}, {int(L)}), not {centres.shape}")
    return np.ascontiguousarray(centres, dtype=np.float64)


def n_iterations(n_iter):
    if isinstance(n_iter, (bool, np.bool_)) or not isinstance(n_iter, (int, np.integer)) or int(n_iter) < 1:
        raise ValueError(f"n_iter must be an integer of at least 1, not {n_iter!r}")
    return int(n_iter)


def host_status(n, status):
    """int32 status (n,) or None: an integer dtype, one value per row (a row whose status is not 0 is no member)"""
    if status is None:
        return None
    status = np.asarray(status)
    if status.dtype.kind not in "iu":
        raise ValueError(f"status must have an integer dtype, not {status.dtype}")
    if status.shape != (int(n),):
        raise ValueError(f"status must hold one value per row: shape ({int(n)},), not {status.shape}")
    return np.ascontiguousarray(status, dtype=np.int32)
