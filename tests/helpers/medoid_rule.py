"""The per-label medoid rule of include/wdx.h (wdx_medoids_device) in NumPy, on the oracle's float32 `dtw_matrix` -- written from
the statement of the rule, not from the kernels:

    member of g      label g, status 0 (if given), all L samples finite
    f(a, b)          the float32 distance of (X[a], X[b]): row a's OWN entry of the oracle's matrix (no symmetry is assumed)
    q_0 < q_1 < ...  the rows of label g in rising row order, members or not; chunk c holds q_{64c} .. q_{64c+63}
    cost[r]          0.0 + S_0 + S_1 + ... in rising c;  S_c = 0.0 + (double)f(r, q_j) over the MEMBERS of chunk c in rising j;
                     NaN for a non-member
    medoid[g]        the member with the smallest cost, the first in row order among equal costs; -1 without a member
    count, medoid_cost, refs (X[medoid] bit for bit, a NaN row without a member)

Sums are strictly sequential (np.add.accumulate; np.sum adds pairwise).  NaN outputs are the quiet NaN 0x7ff8000000000000, so
that cost and refs can be compared bit for bit.  Only the label's own |g| x |g| matrices are computed."""
import numpy as np

QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
CHUNK = 64


def _oracle_matrix(window, penalty):
    from oracle import wdx_oracle as orc

    return lambda A: orc.dtw_matrix(A, A, window, penalty)


def _seq_sum(v):
    """0.0 + v[0] + v[1] + ... along the last axis, in that order (float64)"""
    v = np.asarray(v, dtype=np.float64)
    if v.shape[-1] == 0:
        return np.zeros(v.shape[:-1], dtype=np.float64)
    return np.add.accumulate(v, axis=-1)[..., -1]


def medoid_rule(X, labels, n_labels, window=None, penalty=None, status=None, matrix=None):
    """-> dict(index int64 (G,), refs float64 (G, L), count int64 (G,), medoid_cost float64 (G,), cost float64 (n,)).
    ``matrix``: A -> float32 (len(A), len(A)) distances of the rows of A against themselves (default: the oracle's)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    n, L = X.shape
    G = int(n_labels)
    matrix = matrix or _oracle_matrix(window, penalty)
    member = np.isfinite(X).all(axis=1) & (labels >= 0)
    if status is not None:
        member &= np.asarray(status) == 0
    cost = np.full(n, QNAN, dtype=np.float64)
    index = np.full(G, -1, dtype=np.int64)
    count = np.zeros(G, dtype=np.int64)
    mcost = np.full(G, QNAN, dtype=np.float64)
    refs = np.full((G, L), QNAN, dtype=np.float64)
    for g in range(G):
        q = np.flatnonzero(labels == g)                 # rising row order, members or not
        mem = member[q]
        count[g] = int(mem.sum())
        if not mem.any():
            continue
        D = matrix(X[q])
        assert D.dtype == np.float32 and D.shape == (len(q), len(q))
        with np.errstate(invalid="ignore", over="ignore"):
            total = np.zeros(len(q), dtype=np.float64)
            for c0 in range(0, len(q), CHUNK):
                cols = c0 + np.flatnonzero(mem[c0:c0 + CHUNK])
                total = total + _seq_sum(D[:, cols].astype(np.float64))   # the chunk sums in rising chunk order
        cost[q[mem]] = total[mem]
        k = int(np.argmin(total[mem]))                  # first minimum (a member's cost is never NaN: its distances are >= 0 or +inf)
        assert not np.isnan(total[mem]).any()
        index[g] = q[mem][k]
        mcost[g] = total[mem][k]
        refs[g] = X[index[g]]
    return dict(index=index, refs=refs, count=count, medoid_cost=mcost, cost=cost)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the input of tests/test_gpu_medoids.py ---------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 129, 200, 0, 1)   # label 7 is empty; label 8 holds one row, whose status is 1: no member


def labelled_rows(L, seed=7):
    """(X (n, L), labels (n,), status (n,), G): labels of SIZES rows in shuffled row order, 6 rows labelled -1; among the rows a
    NaN row (label 4), a row with an infinite sample (label 5), a row with status 1 (label 6), and label 8's only row with
    status 1."""
    rng = np.random.default_rng(seed + L)
    lab = np.concatenate([np.full(m, g) for g, m in enumerate(SIZES)] + [np.full(6, -1)]).astype(np.int32)
    rng.shuffle(lab)
    n, G = lab.size, len(SIZES)
    X = np.empty((n, L))
    for g in list(range(G)) + [-1]:
        q = np.flatnonzero(lab == g)
        centre = np.cumsum(rng.normal(0, 0.6, L))
        centre = (centre - centre.mean()) / (centre.std() + 1e-9)
        X[q] = centre + rng.normal(0, 0.35, (len(q), L))
    status = np.zeros(n, dtype=np.int32)
    X[np.flatnonzero(lab == 4)[10], L // 3] = np.nan
    X[np.flatnonzero(lab == 5)[77], L - 1] = np.inf
    status[np.flatnonzero(lab == 6)[5]] = 1
    status[np.flatnonzero(lab == 8)[0]] = 1
    return X, lab, status, G


def tied_rows(L, window, penalty):
    """(X (n, L), labels (n,), G, first, second): label 0 holds 66 rows over two chunks whose two central rows -- the oracle's medoid
    of the other 64 and a copy of it inserted further down -- are identical, so that their costs are equal term by term; label 1
    holds a few rows of its own.  first < second are the rows of the two."""
    X, lab, _, _ = labelled_rows(L)
    rows = X[lab == 6][:65]
    rows = rows[np.isfinite(rows).all(axis=1)][:64]
    m = int(medoid_rule(rows, np.zeros(64, dtype=np.int32), 1, window, penalty)["index"][0])
    second = 64 if m < 40 else 50                       # (in the other chunk, or in the same one)
    rows = np.insert(rows, second, rows[m], axis=0)
    first = m if m < second else m + 1
    first, second = min(first, second), max(first, second)
    other = X[lab == 2][:5]
    return np.concatenate([other[:2], rows, other[2:]]), np.r_[1, 1, np.zeros(65, dtype=np.int32), 1, 1, 1].astype(np.int32), 2, first + 2, second + 2
