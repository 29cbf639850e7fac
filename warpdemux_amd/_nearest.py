"""Arguments of the nearest-reference rule (include/wdx.h: wdx_nearest_dev), checked on the host once for every Python way in:
`parallel_distances.nearest_label`, `DemuxEngine.nearest` and `DemuxEngine.demux_nearest`.  Nothing here touches a GPU."""
from __future__ import annotations

import numpy as np


def n_labels_of(nY, labels, n_labels):
    """G of a call: ``n_labels`` as given, else the references' count (identity labels) or the largest label + 1."""
    if n_labels is None:
        return int(nY) if labels is None else int(np.max(labels)) + 1 if np.size(labels) else 0
    if isinstance(n_labels, (bool, np.bool_)) or not isinstance(n_labels, (int, np.integer)):
        raise ValueError(f"n_labels must be an integer, not {n_labels!r}")
    return int(n_labels)


def host_labels(nY, labels, n_labels):
    """(int32 labels (nY,) or None, G) of host labels: an integer dtype, one label per reference, every label in 0 .. G-1;
    without labels (the identity) G must be the number of references."""
    if labels is not None:
        labels = np.asarray(labels)
        if labels.dtype.kind not in "iu":
            raise ValueError(f"labels must have an integer dtype, not {labels.dtype}")
        if labels.shape != (int(nY),):
            raise ValueError(f"labels must hold one label per reference: shape ({int(nY)},), not {labels.shape}")
    G = n_labels_of(nY, labels, n_labels)
    if G < 1:
        raise ValueError(f"n_labels must be at least 1, not {G}")
    if labels is None:
        if G != int(nY):
            raise ValueError(f"without labels n_labels ({G}) must be the number of references ({int(nY)})")
        return None, G
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= G):
        raise ValueError(f"labels must lie in 0 .. {G - 1}")
    return np.ascontiguousarray(labels, dtype=np.int32), G


def host_threshold(name, t, G):
    """float32 (G,) thresholds from a scalar or one value per label (None stays None)"""
    if t is None:
        return None
    t = np.asarray(t)
    if t.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be real numbers, not {t.dtype}")
    if t.ndim == 0:
        t = np.full(G, t)
    if t.shape != (G,):
        raise ValueError(f"{name} must hold one threshold per label: shape ({G},), not {t.shape}")
    return np.ascontiguousarray(t, dtype=np.float32)
