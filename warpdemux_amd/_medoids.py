"""Arguments of the per-label medoid rule (include/wdx.h: wdx_medoids_device), checked on the host once for both Python ways in:
`parallel_distances.label_medoids` and `DemuxEngine.medoids`.  Nothing here touches a GPU."""
from __future__ import annotations

import numpy as np

from . import _lib


def host_labels(n, labels, n_labels):
    """(int32 labels (n,), G): an integer dtype, one label per row, every label in -1 .. G-1 (-1: the row takes no part);
    ``n_labels`` None: the largest label + 1 (at least 1).  A label of more than `_lib.MEDOID_MAX_GROUP` rows is
    NotImplementedError: the caller subsamples."""
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
    if labels.size:
        sizes = np.bincount(labels[labels >= 0], minlength=G)
        g = int(np.argmax(sizes))
        if sizes[g] > _lib.MEDOID_MAX_GROUP:
            raise NotImplementedError(f"medoids: label {g} has {int(sizes[g])} rows, more than WDX_MEDOID_MAX_GROUP = "
                                      f"{_lib.MEDOID_MAX_GROUP}: subsample it")
    return labels, G


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
