"""The nearest-reference rule of include/wdx.h (wdx_nearest_dev) in NumPy, on a float32 (n, nY) distance matrix -- written from
the statement of the rule (whole columns at a time), not from the kernels:

    c1 = np.argmin(d)  (first minimum; a first NaN wins outright),  lab = g[c1],  d1 = d[c1]
    d2 = min(d[c] for c with g[c] != lab): +inf when no reference has another label, NaN when the row holds a NaN
    margin = d2 - d1 in float32 (inf - inf is NaN)
    call = lab, but -1 when d1 is NaN, when !(margin >= min_margin[lab]) or when !(d1 <= max_dist[lab])
    status != 0: call = -1, d1 = d2 = NaN
    counts int64[G + 1]: bin lab of the accepted reads, bin G of every call of -1

NaN outputs are the quiet NaN 0x7fc00000, so that `best` can be compared bit for bit."""
import numpy as np

QNAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def nearest_rule(D, labels=None, n_labels=None, min_margin=None, max_dist=None, status=None):
    """-> (call int32 (n,), best float32 (n, 2), counts int64 (G + 1,))"""
    D = np.asarray(D)
    assert D.dtype == np.float32 and D.ndim == 2
    n, nY = D.shape
    g = np.arange(nY, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    G = int(n_labels) if n_labels is not None else (nY if labels is None else int(g.max()) + 1)
    assert g.shape == (nY,) and nY >= 1 and G >= 1
    g = np.where((g >= 0) & (g < G), g, G)          # (device labels outside 0 .. G-1: one group of its own, called -1)
    mm = None if min_margin is None else np.broadcast_to(np.asarray(min_margin, dtype=np.float32), (G,))
    md = None if max_dist is None else np.broadcast_to(np.asarray(max_dist, dtype=np.float32), (G,))
    counts = np.zeros(G + 1, dtype=np.int64)
    if n == 0:
        return np.empty(0, dtype=np.int32), np.empty((0, 2), dtype=np.float32), counts
    rows = np.arange(n)
    c1 = np.argmin(D, axis=1)                       # first minimum; a first NaN wins outright
    lab = g[c1]
    d1 = D[rows, c1]
    other = g[None, :] != lab[:, None]              # the references of another label
    d2 = np.where(other, D, np.float32(np.inf)).min(axis=1).astype(np.float32)   # +inf when there is none
    has_nan = np.isnan(D).any(axis=1)
    d1 = np.where(has_nan, QNAN, d1).astype(np.float32)
    d2 = np.where(has_nan, QNAN, d2).astype(np.float32)
    with np.errstate(invalid="ignore"):
        margin = d2 - d1                            # float32; inf - inf is NaN
        inside = lab < G
        li = np.where(inside, lab, 0)
        reject = ~inside | np.isnan(d1)
        if mm is not None:
            reject |= ~(margin >= mm[li])
        if md is not None:
            reject |= ~(d1 <= md[li])
    if status is not None:
        failed = np.asarray(status) != 0
        reject |= failed
        d1 = np.where(failed, QNAN, d1).astype(np.float32)
        d2 = np.where(failed, QNAN, d2).astype(np.float32)
    call = np.where(reject, -1, lab).astype(np.int32)
    best = np.ascontiguousarray(np.stack([d1, d2], axis=1), dtype=np.float32)
    counts += np.bincount(np.where(reject, G, li), minlength=G + 1)
    # (assignments of a NaN scalar keep its payload on every platform NumPy runs on; make it certain)
    bits = best.view(np.uint32)
    bits[np.isnan(best)] = 0x7FC00000
    return call, best, counts


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
