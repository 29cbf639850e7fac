"""The leave-one-out nearest-neighbour rule of include/wdx.h (wdx_self_nearest_device) in NumPy, on the oracle's float32
`dtw_matrix` of the members -- written from the statement of the rule, not from the kernels:

    member           label >= 0, status 0 (if given), all L samples finite
    f(a, b)          row a's OWN entry of the oracle's matrix of the members against the members (no symmetry is assumed)
    own candidates   of a member a: the members b != a with label[b] == label[a];  other candidates: label[b] != label[a]
    nn, best         per side the candidate with the smallest f(a, b) and that f; among equal distances the lowest row index
                     (also when all are +inf); no candidate: -1, +inf;  a non-member: -1, the quiet NaN 0x7fc00000 on both sides

Only the members' matrix is computed."""
import numpy as np

from helpers.self_matrix_rule import QNAN32, bits, same_bits  # noqa: F401  (the tests compare with them)

N_ROWS = 200   # four chunks of 64 rows, the last partial


def members(X, labels=None, status=None):
    m = np.isfinite(np.asarray(X, dtype=np.float64)).all(axis=1)
    if labels is not None:
        m &= np.asarray(labels) >= 0
    if status is not None:
        m &= np.asarray(status) == 0
    return m


def rule_on_matrix(D, labels, mem):
    """(nn int32 (n, 2), best float32 (n, 2)) from a float32 (n, n) matrix whose entry (a, b) is f(a, b) wherever a and b are both
    members (anything elsewhere), the labels (None: all 0) and the member flags"""
    D = np.asarray(D)
    n = D.shape[0]
    assert D.dtype == np.float32 and D.shape == (n, n)
    lab = np.zeros(n, dtype=np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    nn = np.full((n, 2), -1, dtype=np.int32)
    best = np.full((n, 2), QNAN32, dtype=np.float32)
    idx = np.arange(n)
    for a in np.flatnonzero(mem):
        for side, cand in enumerate((mem & (lab == lab[a]) & (idx != a), mem & (lab != lab[a]))):
            q = np.flatnonzero(cand)
            if q.size == 0:
                best[a, side] = np.inf
                continue
            row = D[a, q]
            assert not np.isnan(row).any(), "f between members is never NaN"
            k = int(np.argmin(row))          # the first minimum: q rises, so the lowest row index (+inf everywhere: the first)
            nn[a, side], best[a, side] = q[k], row[k]
    return nn, best


def loo_rule(X, labels=None, window=None, penalty=None, status=None, matrix=None):
    """-> (nn int32 (n, 2), best float32 (n, 2)).  ``matrix``: (A, B) -> float32 (len(A), len(B)) distances (default: the oracle's)."""
    if matrix is None:
        from oracle import wdx_oracle as orc

        matrix = lambda A, B: orc.dtw_matrix(A, B, window, penalty)   # noqa: E731
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    mem = members(X, labels, status)
    q = np.flatnonzero(mem)
    D = np.zeros((n, n), dtype=np.float32)
    if q.size:
        M = np.ascontiguousarray(X[q])
        Dm = matrix(M, M)
        assert Dm.dtype == np.float32 and Dm.shape == (q.size, q.size)
        D[np.ix_(q, q)] = Dm
    return rule_on_matrix(D, labels, mem)


def tie_cells(X, labels, window, penalty, status=None):
    """number of (row, side) cells whose minimum is reached by more than one candidate (oracle's distances)"""
    from oracle import wdx_oracle as orc

    X = np.ascontiguousarray(X, dtype=np.float64)
    mem = members(X, labels, status)
    q = np.flatnonzero(mem)
    lab = np.asarray(labels)[q]
    D = orc.dtw_matrix(np.ascontiguousarray(X[q]), np.ascontiguousarray(X[q]), window, penalty)
    cells = 0
    for i in range(q.size):
        for cand in ((lab == lab[i]) & (np.arange(q.size) != i), lab != lab[i]):
            row = D[i, cand]
            cells += int(row.size > 1 and (row == row.min()).sum() > 1)
    return cells


# ---- the input of tests/test_gpu_loo.py and tests/test_loo_host.py ---------------------------------------------------------------
def rows(L, n=N_ROWS, seed=29):
    """(X (n, L), labels (n,), status (n,)): rows around five random-walk centres, label = the centre, noise 0.35.  From n = 130 on:
    a NaN sample (row 14), an infinite sample (90), status 1 (195), label -1 (50); four mislabelled rows (20, 60, 140, 180: the next
    label); rows 80 and 160 copies of row 10 with its label, rows 110 and 194 copies of row 10 with another label (exact ties at
    distance 0 on both sides); row 120 the only row of label 5 (no own candidate); row 100 scaled by 1e160, so that every distance
    to it overflows to +inf.  With n = 200 the changed rows span all four chunks."""
    rng = np.random.default_rng(seed + L)
    centres = np.cumsum(rng.normal(0, 0.6, (5, L)), axis=1)
    centres = (centres - centres.mean(axis=1, keepdims=True)) / (centres.std(axis=1, keepdims=True) + 1e-9)
    labels = rng.integers(0, 5, n).astype(np.int32)
    X = centres[labels] + rng.normal(0, 0.35, (n, L))
    status = np.zeros(n, dtype=np.int32)
    if n >= 130:
        for r in (20, 60, 140, 180):
            if r < n:
                labels[r] = (labels[r] + 1) % 5
        for r in (80, 160):
            if r < n:
                X[r], labels[r] = X[10], labels[10]
        for r in (110, 194):
            if r < n:
                X[r], labels[r] = X[10], (labels[10] + 2) % 5
        labels[120] = 5
        X[100] *= 1e160
        X[14, L // 3] = np.nan
        X[90, L - 1] = np.inf
        labels[50] = -1
        if 195 < n:
            status[195] = 1
    return X, labels, status
