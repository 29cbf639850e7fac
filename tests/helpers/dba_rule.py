"""One barycenter step as include/wdx.h states it (wdx_dba_step_device), in NumPy float64 -- written from the statement of the
rule, not from the kernels:

    member of g      label g, status 0 (if given), all L samples finite; a label whose centre holds a sample that is not finite,
                     or which has no member, is idle
    D                D[0][0] = 0, +inf elsewhere; inside the band  t = min(D[i][j+1], D[i+1][j]) + p2,
                     D[i+1][j+1] = (x[i] - c[j])^2 + min(t, D[i][j]) -- every operation rounded on its own; cost = D[L][L]
    direction        diag if D[i][j] <= t, else up if D[i][j+1] <= D[i+1][j], else left; at i == 0 left, at j == 0 up
    runs             the rows the path from (L-1, L-1) to (0, 0) matches to column j: lo[j] .. hi[j]
    sums             s_r[j] = x[lo] + ... + x[hi] in rising i; S_c[j] over the members of chunk c (64 rows of the label in rising row
                     order, members or not) in rising order; T[j] = S_0[j] + S_1[j] + ...; K[j] the integer sum of the run lengths;
                     new centre T[j] / K[j]; inertia the same two-level sum of cost

Sums are strictly sequential (np.add.accumulate; np.sum adds pairwise) and start at 0.0.  NaN outputs are the quiet NaN.  The rows
of one label are walked together: the Python loops run over cells and path steps, the arrays over rows."""
import numpy as np

from .medoid_rule import CHUNK, QNAN, _seq_sum

DIAG, UP, LEFT = 0, 1, 2


def effective_window(L, window):
    return L if (not window or window <= 0 or window > L) else int(window)


def cost_matrix(X, c, window=None, penalty=None):
    """(D (m, L+1, L+1) float64, direction (m, L, L) int8, -1 outside the band) of the rows of X against one centre c"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    m, L = X.shape
    w = effective_window(L, window)
    pen = np.float64(penalty if penalty else 0.0)
    p2 = pen * pen
    D = np.full((m, L + 1, L + 1), np.inf)
    D[:, 0, 0] = 0.0
    direction = np.full((m, L, L), -1, dtype=np.int8)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(L):
            for j in range(max(0, i - (w - 1)), min(L - 1, i + (w - 1)) + 1):
                d = X[:, i] - c[j]
                diag, up, left = D[:, i, j], D[:, i, j + 1], D[:, i + 1, j]
                t = np.minimum(up, left) + p2
                D[:, i + 1, j + 1] = d * d + np.minimum(t, diag)
                k = np.where(diag <= t, DIAG, np.where(up <= left, UP, LEFT))
                if i == 0:
                    k = np.full(m, LEFT)
                if j == 0:
                    k = np.full(m, UP)
                direction[:, i, j] = k
    return D, direction


def walk(direction, want_steps=False):
    """(lo, hi) int32 (m, L) of the paths from (L-1, L-1) to (0, 0)[, the visited cells per row as a list of (i, j, code)]"""
    m, L, _ = direction.shape
    rows = np.arange(m)
    i = np.full(m, L - 1)
    j = np.full(m, L - 1)
    lo = np.full((m, L), L, dtype=np.int32)
    hi = np.full((m, L), -1, dtype=np.int32)
    steps = []
    for _ in range(2 * L):
        lo[rows, j] = np.minimum(lo[rows, j], i)
        hi[rows, j] = np.maximum(hi[rows, j], i)
        live = (i > 0) | (j > 0)
        if not live.any():
            break
        k = direction[rows, i, j]
        assert (k[live] >= 0).all(), "the path left the band"
        if want_steps:
            steps.append((i.copy(), j.copy(), np.where(live, k, -1)))
        i = np.where(live & (k != LEFT), i - 1, i)
        j = np.where(live & (k != UP), j - 1, j)
    else:
        raise AssertionError("a path did not reach (0, 0)")
    return (lo, hi, steps) if want_steps else (lo, hi)


def run_sums(X, lo, hi):
    """s_r (m, L) float64: x[lo[j]] + ... + x[hi[j]], from 0.0 in rising i"""
    m, L = X.shape
    s = np.zeros((m, L))
    rows = np.arange(m)[:, None]
    for k in range(int((hi - lo).max()) + 1 if m else 0):
        at = lo + k
        use = at <= hi
        s = np.where(use, s + X[rows, np.minimum(at, L - 1)], s)
    return s


def align(X, c, window=None, penalty=None):
    """dict(cost (m,), lo, hi (m, L) int32, s (m, L)) of finite rows X against the finite centre c"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    D, direction = cost_matrix(X, c, window, penalty)
    lo, hi = walk(direction)
    return dict(cost=D[:, -1, -1].copy(), lo=lo, hi=hi, s=run_sums(X, lo, hi))


def average(s, lo, hi, cost, where, size):
    """(new centre (L,), inertia) of one label from its members' run sums s (m, L), runs and costs: ``where`` is each member's place
    among the label's ``size`` rows (rising row order, members or not); chunk sums over the members of 64 places in rising order, then
    the chunks in rising order"""
    L = s.shape[1]
    k = (hi - lo + 1).astype(np.int64)
    T, K, I = np.zeros(L), np.zeros(L, dtype=np.int64), np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for c0 in range(0, size, CHUNK):
            sel = (where >= c0) & (where < c0 + CHUNK)
            T = T + _seq_sum(s[sel].T)                  # S_c[j]: the members of the chunk in rising order
            I = I + _seq_sum(cost[sel])
            K = K + k[sel].sum(axis=0)
        return T / K.astype(np.float64), I


def dba_step(X, labels, centres, n_labels=None, window=None, penalty=None, status=None):
    """-> dict(new_centres (G, L) float64, count int64 (G,), inertia float64 (G,), cost float64 (n,), runs int32 (n, L, 2))"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    centres = np.ascontiguousarray(centres, dtype=np.float64)
    n, L = X.shape
    G = int(n_labels) if n_labels is not None else len(centres)
    assert centres.shape == (G, L)
    member = np.isfinite(X).all(axis=1) & (labels >= 0)
    if status is not None:
        member &= np.asarray(status) == 0
    new = np.full((G, L), QNAN)
    count = np.zeros(G, dtype=np.int64)
    inertia = np.full(G, QNAN)
    cost = np.full(n, QNAN)
    runs = np.full((n, L, 2), -1, dtype=np.int32)
    for g in range(G):
        q = np.flatnonzero(labels == g)                 # rising row order, members or not
        mem = member[q]
        if not mem.any() or not np.isfinite(centres[g]).all():
            continue                                    # idle
        a = align(X[q[mem]], centres[g], window, penalty)
        cost[q[mem]] = a["cost"]
        runs[q[mem], :, 0], runs[q[mem], :, 1] = a["lo"], a["hi"]
        count[g] = int(mem.sum())
        new[g], inertia[g] = average(a["s"], a["lo"], a["hi"], a["cost"], np.flatnonzero(mem), len(q))
    return dict(new_centres=new, count=count, inertia=inertia, cost=cost, runs=runs)


def tied_input(L, seed=11):
    """(X (n, L), labels (n,), centres (G, L), G): rows and centres drawn from {-1, 0, 1}, so that equal predecessors abound; labels
    of 70, 64 and 5 rows in shuffled row order and 3 rows labelled -1"""
    rng = np.random.default_rng(seed + L)
    lab = np.concatenate([np.full(70, 0), np.full(64, 1), np.full(5, 2), np.full(3, -1)]).astype(np.int32)
    rng.shuffle(lab)
    X = rng.integers(-1, 2, (lab.size, L)).astype(np.float64)
    C = rng.integers(-1, 2, (3, L)).astype(np.float64)
    return X, lab, C, 3


def tied_share(X, c, window=None, penalty=None):
    """share of the path steps of the rows of X against c that sit on a tied cell: diag == t, or (diag > t and up == left)"""
    D, direction = cost_matrix(X, c, window, penalty)
    _, _, steps = walk(direction, want_steps=True)
    pen = np.float64(penalty if penalty else 0.0)
    rows = np.arange(len(X))
    tied = total = 0
    for i, j, k in steps:
        live = k >= 0
        diag, up, left = D[rows, i, j], D[rows, i, j + 1], D[rows, i + 1, j]
        t = np.minimum(up, left) + pen * pen
        tie = (diag == t) | ((diag > t) & (up == left))
        tied += int((tie & live).sum())
        total += int(live.sum())
    return tied / max(total, 1)


def barycenters(X, labels, init, n_labels=None, window=None, penalty=None, status=None, n_iter=10):
    """(centres, count, inertia (steps, G)): at most n_iter steps from `init`, stopping when a step returns its input bit for bit"""
    C = np.ascontiguousarray(init, dtype=np.float64).copy()
    hist, count = [], None
    for _ in range(n_iter):
        r = dba_step(X, labels, C, n_labels, window, penalty, status)
        hist.append(r["inertia"])
        count = r["count"]
        same = np.array_equal(r["new_centres"].view(np.uint64), C.view(np.uint64))
        C = r["new_centres"]
        if same:
            break
    return C, count, np.array(hist).reshape(len(hist), -1)
