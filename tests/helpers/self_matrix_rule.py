"""The self-distance matrix rule of include/wdx.h (wdx_self_matrix_device) in NumPy, on the oracle's float32 `dtw_matrix` --
written from the statement of the rule, not from the kernels:

    member           status 0 (if given), all L samples finite
    out[a, b]        float32, 0 <= a, b < n
                     both members: f(a, b), the float32 distance of (X[a], X[b]) -- row a's OWN entry of the oracle's matrix of
                     the members against the members (no symmetry is assumed in the expectation)
                     otherwise: the quiet NaN 0x7fc00000

Only the members' matrix is computed."""
import numpy as np

QNAN32 = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def members(X, status=None):
    m = np.isfinite(np.asarray(X, dtype=np.float64)).all(axis=1)
    if status is not None:
        m &= np.asarray(status) == 0
    return m


def self_matrix_rule(X, window=None, penalty=None, status=None, matrix=None):
    """-> float32 (n, n).  ``matrix``: (A, B) -> float32 (len(A), len(B)) distances (default: the oracle's)."""
    if matrix is None:
        from oracle import wdx_oracle as orc

        matrix = lambda A, B: orc.dtw_matrix(A, B, window, penalty)   # noqa: E731
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    mem = members(X, status)
    out = np.full((n, n), QNAN32, dtype=np.float32)
    q = np.flatnonzero(mem)
    if q.size:
        M = np.ascontiguousarray(X[q])
        D = matrix(M, M)
        assert D.dtype == np.float32 and D.shape == (q.size, q.size)
        out[np.ix_(q, q)] = D
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the inputs of tests/test_gpu_self_matrix.py ------------------------------------------------------------------------------
N_ROWS = 200   # four chunks of 64 rows, the last partial: 4 diagonal and 6 strictly upper tiles


def rows(L, n=N_ROWS, seed=11):
    """(X (n, L), status (n,)): rows around five centres; among them (where n allows) a NaN row, a row with an infinite sample
    and a row with status 1 -- in different chunks when n = 200."""
    rng = np.random.default_rng(seed + L)
    centres = np.cumsum(rng.normal(0, 0.6, (5, L)), axis=1)
    centres = (centres - centres.mean(axis=1, keepdims=True)) / (centres.std(axis=1, keepdims=True) + 1e-9)
    X = centres[rng.integers(0, 5, n)] + rng.normal(0, 0.35, (n, L))
    status = np.zeros(n, dtype=np.int32)
    if n >= 3:
        X[(n * 7) // 100, L // 3] = np.nan       # n = 200: row 14, chunk 0
        X[(n * 45) // 100, L - 1] = np.inf       # row 90, chunk 1
        status[n - 1 - n // 50] = 1              # row 195, the partial chunk
    return X, status


def training_rows(k, n_train, L, seed, n_test=256):
    """(Xtr, ytr, Xte, yte): ``centers[y] + 0.6 * noise`` as tests/test_gpu_live.py's _svm_model draws its training set, then n_test
    held-out rows of the same centres from the same generator"""
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(k, L))
    y = rng.integers(0, k, n_train)
    Xtr = centers[y] + 0.6 * rng.normal(size=(n_train, L))
    yte = rng.integers(0, k, n_test)
    Xte = centers[yte] + 0.6 * rng.normal(size=(n_test, L))
    return Xtr, y, Xte, yte
