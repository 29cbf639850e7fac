"""The rule of the batched SMO solver (include/wdx.h: wdx_svm_solve_device, steps 1 to 8) restated in NumPy: the device kernel is
held to it bit for bit (tests/test_gpu_svm_fit.py), and it is itself compared with scikit-learn's libsvm through the KKT conditions
and the dual objective (tests/test_svm_solver_host.py).

NumPy's element-wise float64 operations round each product, sum and quotient on its own (no ufunc fuses a multiply into an add),
`np.argmax` returns the lowest index of the maximum, and the two sequential sums of step 8 are `np.cumsum`'s (strictly left to
right) and a Python loop.  K is read through the index list exactly as the kernel reads it: rows i and j of an iteration, and the
diagonal once.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

TAU = 1e-12
QNAN = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), dtype=np.float64)[0]


class Solve(NamedTuple):
    alpha: np.ndarray
    rho: float
    n_iter: int
    state: int
    dec: np.ndarray


def default_max_iter(rows):
    return max(10_000_000, 100 * int(rows))


def solve(K, rows, n_pos, c_pos, c_neg, eps=1e-3, max_iter=None, eval_rows=(), stats=None):
    """One problem.  K: float32 (m, >= m); rows: the K rows of the problem, the first n_pos with y = +1.  ``stats``: a dict that
    receives how many pairs took the TAU branch of step 6 ("tau") and whether rho is the midpoint form ("midpoint")."""
    rows = np.asarray(rows, dtype=np.int64)
    n = len(rows)
    pos = np.arange(n) < n_pos
    y = np.where(pos, 1.0, -1.0)
    C = np.where(pos, float(c_pos), float(c_neg))
    kd = K[rows, rows].astype(np.float64)
    a, G = np.zeros(n), -np.ones(n)
    max_iter = default_max_iter(n) if max_iter is None else int(max_iter)
    it, state, gmax, gmin = 0, 0, 0.0, 0.0
    with np.errstate(all="ignore"):
        while True:
            if not np.isfinite(G).all():                                           # 2
                state = 2
                break
            v = -y * G
            up = np.where(pos, a < C, a > 0)                                       # 3
            low = np.where(pos, a > 0, a < C)
            vi = np.where(up, v, -np.inf)                                          # 4
            i = int(np.argmax(vi))
            gmax = vi[i]
            gmin = np.where(low, v, np.inf).min()
            if gmax - gmin < eps:
                break
            if it == max_iter:
                state = 1
                break
            Ki = K[rows[i], rows].astype(np.float64)                               # 5
            b = gmax - v
            c = (kd[i] + kd) - 2.0 * Ki
            c = np.where(c > 0, c, TAU)
            score = np.where(low & (b > 0), (b * b) / c, -np.inf)
            score = np.where(np.isnan(score), -np.inf, score)
            j = int(np.argmax(score))
            if not score[j] > -np.inf:
                state = 2
                break
            Ci, Cj, oi, oj = C[i], C[j], a[i], a[j]                                # 6
            q = (kd[i] + kd[j]) - 2.0 * Ki[j]
            if stats is not None and not q > 0:
                stats["tau"] = stats.get("tau", 0) + 1
            q = q if q > 0 else TAU
            if y[i] != y[j]:
                d = (-G[i] - G[j]) / q
                diff = a[i] - a[j]
                a[i] += d
                a[j] += d
                if diff > 0:
                    if a[j] < 0:
                        a[j], a[i] = 0.0, diff
                else:
                    if a[i] < 0:
                        a[i], a[j] = 0.0, -diff
                if diff > Ci - Cj:
                    if a[i] > Ci:
                        a[i], a[j] = Ci, Ci - diff
                else:
                    if a[j] > Cj:
                        a[j], a[i] = Cj, Cj + diff
            else:
                d = (G[i] - G[j]) / q
                s = a[i] + a[j]
                a[i] -= d
                a[j] += d
                if s > Ci:
                    if a[i] > Ci:
                        a[i], a[j] = Ci, s - Ci
                else:
                    if a[j] < 0:
                        a[j], a[i] = 0.0, s
                if s > Cj:
                    if a[j] > Cj:
                        a[j], a[i] = Cj, s - Cj
                else:
                    if a[i] < 0:
                        a[i], a[j] = 0.0, s
            Kj = K[rows[j], rows].astype(np.float64)                               # 7
            G = G + ((y * y[i] * Ki) * (a[i] - oi) + (y * y[j] * Kj) * (a[j] - oj))
            it += 1
        ev = np.asarray(eval_rows, dtype=np.int64)
        if state == 2:                                                             # 8
            return Solve(a, QNAN, it, state, np.full(len(ev), QNAN))
        free = (a > 0) & (a < C)
        if stats is not None:
            stats["midpoint"] = not free.any()
        if free.any():
            rho = -np.cumsum((-y * G)[free])[-1] / float(free.sum())
        else:
            rho = -(gmax + gmin) / 2.0
        dec = np.zeros(len(ev))
        coef = a * y
        for s_ in np.flatnonzero(a > 0):
            dec = dec + coef[s_] * K[ev, rows[s_]].astype(np.float64)
        return Solve(a, float(rho), it, state, dec - rho)


def solve_batch(K, batch, eps, max_iter):
    """`warpdemux_amd._svm_fit.Solution` of a `Batch`, every problem through `solve`: the solver argument of `_svm_fit.fit_arrays`."""
    from warpdemux_amd._svm_fit import Solution

    Q = len(batch.problems)
    out = Solution(np.zeros(len(batch.rows)), np.empty(Q), np.empty(Q, np.int64), np.empty(Q, np.int32), np.zeros(len(batch.eval_rows)))
    for q, pr in enumerate(batch.problems):
        r0, e0, n = int(pr["row0"]), int(pr["eval0"]), int(pr["n_pos"]) + int(pr["n_neg"])
        s = solve(K, batch.rows[r0:r0 + n], int(pr["n_pos"]), pr["c_pos"], pr["c_neg"], eps, max_iter, batch.eval_rows[e0:e0 + int(pr["n_eval"])])
        out.alpha[r0:r0 + n], out.rho[q], out.n_iter[q], out.state[q] = s.alpha, s.rho, s.n_iter, s.state
        out.dec[e0:e0 + int(pr["n_eval"])] = s.dec
    return out


def objective(K, rows, n_pos, alpha):
    """The dual objective 1/2 a'Qa - e'a of a problem's alpha."""
    rows = np.asarray(rows, dtype=np.int64)
    y = np.where(np.arange(len(rows)) < n_pos, 1.0, -1.0)
    ay = alpha * y
    return 0.5 * float(ay @ (K[np.ix_(rows, rows)].astype(np.float64) @ ay)) - float(alpha.sum())


def kkt_worst(K, rows, n_pos, c_pos, c_neg, alpha, rho):
    """The largest violation of the three KKT conditions of tests/helpers/kkt.py over ALL rows of a problem (support rows or
    not), with the same bound classification: free |y f - 1|, at C: y f - 1, at 0: -(y f - 1)."""
    rows = np.asarray(rows, dtype=np.int64)
    pos = np.arange(len(rows)) < n_pos
    y, C = np.where(pos, 1.0, -1.0), np.where(pos, float(c_pos), float(c_neg))
    f = K[np.ix_(rows, rows)].astype(np.float64) @ (alpha * y) - rho
    r = y * f - 1.0
    zero, bound = alpha <= 1e-12, alpha >= C * (1.0 - 1e-9)
    free = ~zero & ~bound
    worst = 0.0
    if free.any():
        worst = max(worst, float(np.abs(r[free]).max()))
    if bound.any():
        worst = max(worst, float(r[bound].max()))
    if zero.any():
        worst = max(worst, float(-r[zero].min()))
    return worst
