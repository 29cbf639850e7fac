"""Host code around the batched SMO solve (include/wdx.h: wdx_svm_solve_device states the solver's rule): what
``models.DTW_SVM.fit(solver="device")`` does between the kernel matrix and the fitted arrays.

One call solves the k (k - 1) / 2 one-vs-one problems of a precomputed-kernel C-SVC and, for each of them, the five fold problems
that libsvm's Platt scaling cross-validates (svm.cpp: svm_binary_svc_probability).  From the folds' held-out decision values
come ``probA`` / ``probB`` (`sigmoid_train`: Lin, Lin, Weng 2007, in NumPy float64); from the full problems libsvm's model layout
(`assemble`).  Nothing here touches a device but `solve_host`; the others take the solver as an argument, so the tests run them on
the NumPy restatement of the rule.

THE FOLDS are this engine's own: scikit-learn draws libsvm's permutation from a C random generator that cannot be reproduced, so
``probA`` / ``probB`` of a device fit differ from those of a libsvm fit of the same data (both are five-fold estimates of the
same sigmoid).  Pair (i, j) takes its member rows in ascending order, permutes them with
``np.random.default_rng([random_state, i, j])``, and fold f holds out entries ``f * n // 5 .. (f + 1) * n // 5`` of the
permutation.  A fold whose training part lacks a side takes libsvm's constants (+1 with only class i left, -1 with only class j,
0 with neither) and is not solved.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _lib

N_FOLDS = 5

# wdx_svm_problem (include/wdx.h)
PROBLEM_DTYPE = np.dtype([("row0", np.int64), ("eval0", np.int64), ("n_pos", np.int32), ("n_neg", np.int32), ("n_eval", np.int32),
                          ("reserved_", np.int32), ("c_pos", np.float64), ("c_neg", np.float64)], align=True)
assert PROBLEM_DTYPE.itemsize == 48


class Batch(NamedTuple):
    """The problems of one fit.  ``kind[q]`` is -1 for a pair's full problem and f for its fold f; ``pair[q]`` its pair's number
    (libsvm's order: (0, 1), (0, 2), ..).  ``held[p]``: per pair the member rows in the order of ``dec_of`` (the permutation),
    ``held_y`` their +1 / -1, ``const[p]`` the folds' constants where a fold is not solved (NaN elsewhere)."""

    problems: np.ndarray
    rows: np.ndarray
    eval_rows: np.ndarray
    pairs: list
    kind: np.ndarray
    pair: np.ndarray
    held: list
    held_y: list
    const: list


class Solution(NamedTuple):
    alpha: np.ndarray    # float64 per entry of Batch.rows
    rho: np.ndarray      # float64 per problem
    n_iter: np.ndarray   # int64 per problem
    state: np.ndarray    # int32 per problem: 0 converged, 1 iteration cap, 2 stopped (non-finite gradient / no second index)
    dec: np.ndarray      # float64 per entry of Batch.eval_rows


def class_weights(class_weight, classes, y_idx):
    """float64 (k,): the weight of each class -- ``None`` 1, ``"balanced"`` n / (k * count) (scikit-learn's rule), a dict by
    class label (a class it does not name: 1)."""
    k = len(classes)
    if class_weight is None:
        return np.ones(k)
    if isinstance(class_weight, str):
        if class_weight != "balanced":
            raise ValueError(f'class_weight must be None, "balanced" or a dict, not {class_weight!r}')
        return len(y_idx) / (k * np.bincount(y_idx, minlength=k).astype(np.float64))
    if not isinstance(class_weight, dict):
        raise ValueError(f'class_weight must be None, "balanced" or a dict, not {type(class_weight).__name__}')
    known = set(int(c) for c in classes)
    for key in class_weight:
        if key not in known:
            raise ValueError(f"class_weight names the label {key!r}, which is not among the members' labels")
    w = np.array([float(class_weight.get(int(c), 1.0)) for c in classes])
    if not (np.isfinite(w).all() and (w > 0).all()):
        raise ValueError("class weights must be positive and finite")
    return w


def effective_max_iter(max_iter, largest_rows):
    """libsvm's own cap for -1: max(10 000 000, 100 * rows)."""
    if max_iter == -1:
        return max(10_000_000, 100 * int(largest_rows))
    if not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError(f"max_iter must be -1 or a non-negative integer, not {max_iter!r}")
    return int(max_iter)


def fold_chunks(members, i, j, random_state):
    """(permutation of the pair's ascending member rows, the five (begin, end) chunks of it)."""
    perm = np.random.default_rng([int(random_state), int(i), int(j)]).permutation(np.sort(np.asarray(members)))
    n = len(perm)
    return perm, [(f * n // N_FOLDS, (f + 1) * n // N_FOLDS) for f in range(N_FOLDS)]


def build_batch(y_idx, k, c_of_class, random_state=0, folds=True) -> Batch:
    """``y_idx``: the class number 0 .. k-1 of every member row; ``c_of_class``: C times the class weight, per class."""
    y_idx = np.asarray(y_idx)
    rows_of = [np.flatnonzero(y_idx == c).astype(np.int32) for c in range(k)]
    problems, rows, evals, pairs, kind, pair_of, held, held_y, const = [], [], [], [], [], [], [], [], []
    n_rows = n_eval = 0

    def add(pos, neg, ev, i, j, what, p):
        nonlocal n_rows, n_eval
        problems.append((n_rows, n_eval, len(pos), len(neg), len(ev), 0, c_of_class[i], c_of_class[j]))
        rows.extend((pos, neg))
        evals.append(ev)
        n_rows += len(pos) + len(neg)
        n_eval += len(ev)
        kind.append(what)
        pair_of.append(p)

    for i in range(k):
        for j in range(i + 1, k):
            p = len(pairs)
            pairs.append((i, j))
            pos, neg = rows_of[i], rows_of[j]
            add(pos, neg, np.zeros(0, np.int32), i, j, -1, p)
            if not folds:
                held.append(np.zeros(0, np.int32)), held_y.append(np.zeros(0)), const.append(np.zeros(0))
                continue
            perm, chunks = fold_chunks(np.concatenate([pos, neg]), i, j, random_state)
            perm = perm.astype(np.int32)
            cst = np.full(len(perm), np.nan)
            for f, (b, e) in enumerate(chunks):
                if b == e:   # (fewer than five rows: this fold holds nothing out)
                    continue
                train = np.sort(np.concatenate([perm[:b], perm[e:]]))
                tp, tn = train[y_idx[train] == i], train[y_idx[train] == j]
                if len(tp) and len(tn):
                    add(tp, tn, perm[b:e], i, j, f, p)
                else:
                    cst[b:e] = 1.0 if len(tp) else (-1.0 if len(tn) else 0.0)
            held.append(perm), held_y.append(np.where(y_idx[perm] == i, 1.0, -1.0)), const.append(cst)
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dtype=np.int32)   # noqa: E731
    return Batch(np.array(problems, dtype=PROBLEM_DTYPE), cat(rows), cat(evals), pairs, np.array(kind, np.int32), np.array(pair_of, np.int32),
                 held, held_y, const)


def check_batch(batch: Batch):
    """NotImplementedError for a problem beyond the solver's row cap -- before any device work."""
    if len(batch.problems):
        n = batch.problems["n_pos"].astype(np.int64) + batch.problems["n_neg"]
        if n.max() > _lib.SVM_FIT_MAX_ROWS:
            q = int(np.argmax(n))
            i, j = batch.pairs[int(batch.pair[q])]
            raise NotImplementedError(f"svm solve: the problem of classes {i} and {j} has {int(n[q])} rows, more than "
                                      f"WDX_SVM_FIT_MAX_ROWS = {_lib.SVM_FIT_MAX_ROWS}: subsample them, or fit with solver='libsvm'")


def solve_host(K, batch: Batch, eps, max_iter, device: Optional[int] = None) -> Solution:
    """The batch on the device through wdx_svm_solve: ``K`` a float32 (m, m) host matrix, one synchronisation."""
    K = np.ascontiguousarray(K, dtype=np.float32)
    m = K.shape[0]
    if K.ndim != 2 or K.shape[1] != m:
        raise ValueError(f"K must be square, not {K.shape}")
    check_batch(batch)
    Q = len(batch.problems)
    out = Solution(np.zeros(len(batch.rows)), np.empty(Q), np.empty(Q, np.int64), np.empty(Q, np.int32), np.zeros(len(batch.eval_rows)))
    ctx = _lib.default_context(device)
    _lib.check(_lib.load().wdx_svm_solve(ctx.handle, _lib.ptr(K), m, m, _lib.ptr(batch.problems), Q, _lib.ptr(batch.rows), len(batch.rows),
                                         _lib.ptr(batch.eval_rows), len(batch.eval_rows), float(eps), int(max_iter), _lib.ptr(out.alpha),
                                         _lib.ptr(out.rho), _lib.ptr(out.n_iter), _lib.ptr(out.state), _lib.ptr(out.dec)))
    return out


def sigmoid_train(dec, y):
    """(A, B) of P(y = +1 | dec) = 1 / (1 + exp(A dec + B)): libsvm's sigmoid_train (Lin, Lin, Weng 2007: Newton's method with
    backtracking on the regularised targets), float64."""
    dec, y = np.asarray(dec, dtype=np.float64), np.asarray(y)
    prior1, prior0 = float((y > 0).sum()), float((y <= 0).sum())
    max_iter, min_step, sigma, eps = 100, 1e-10, 1e-12, 1e-5
    hi, lo = (prior1 + 1.0) / (prior1 + 2.0), 1.0 / (prior0 + 2.0)
    t = np.where(y > 0, hi, lo)
    A, B = 0.0, float(np.log((prior0 + 1.0) / (prior1 + 1.0)))

    def objective(a, b):
        f = dec * a + b
        return float(np.sum(np.where(f >= 0, t * f + np.log1p(np.exp(-np.abs(f))), (t - 1.0) * f + np.log1p(np.exp(-np.abs(f))))))

    fval = objective(A, B)
    for _ in range(max_iter):
        f = dec * A + B
        e = np.exp(-np.abs(f))
        p = np.where(f >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
        q = np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        d2 = p * q
        h11, h22, h21 = sigma + float(np.sum(dec * dec * d2)), sigma + float(np.sum(d2)), float(np.sum(dec * d2))
        d1 = t - p
        g1, g2 = float(np.sum(dec * d1)), float(np.sum(d1))
        if abs(g1) < eps and abs(g2) < eps:
            break
        det = h11 * h22 - h21 * h21
        dA, dB = -(h22 * g1 - h21 * g2) / det, -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        step = 1.0
        while step >= min_step:
            nA, nB = A + step * dA, B + step * dB
            nf = objective(nA, nB)
            if nf < fval + 0.0001 * step * gd:
                A, B, fval = nA, nB, nf
                break
            step /= 2.0
        if step < min_step:   # (the line search fails: libsvm stops here too)
            break
    return A, B


def assemble(y_idx, k, batch: Batch, sol: Solution):
    """libsvm's model layout from the full problems: (n_support int32 (k,), support int32 (nSV,), dual_coef float64 (k-1, nSV),
    rho float64 (pairs,)).  A support row is a row with alpha > 0 in any pair; they are grouped by class, in ascending row order;
    pair (i, j) puts class i's coefficients (+alpha) into row j - 1 and class j's (-alpha) into row i."""
    y_idx = np.asarray(y_idx)
    n = len(y_idx)
    full = np.flatnonzero(batch.kind == -1)
    alpha_of = []
    is_sv = np.zeros(n, dtype=bool)
    for q in full:
        pr = batch.problems[q]
        a = sol.alpha[pr["row0"]: pr["row0"] + pr["n_pos"] + pr["n_neg"]]
        r = batch.rows[pr["row0"]: pr["row0"] + pr["n_pos"] + pr["n_neg"]]
        alpha_of.append((r, a, int(pr["n_pos"])))
        is_sv[r[a > 0]] = True
    support = np.concatenate([np.flatnonzero(is_sv & (y_idx == c)) for c in range(k)]).astype(np.int32)
    n_support = np.array([int((is_sv & (y_idx == c)).sum()) for c in range(k)], dtype=np.int32)
    where = np.full(n, -1, dtype=np.int64)
    where[support] = np.arange(len(support))
    dual = np.zeros((k - 1, len(support)))
    for (i, j), (r, a, n_pos) in zip(batch.pairs, alpha_of):
        sv = is_sv[r]
        pos = np.arange(len(r)) < n_pos
        dual[j - 1, where[r[sv & pos]]] = a[sv & pos]
        dual[i, where[r[sv & ~pos]]] = -a[sv & ~pos]
    return n_support, support, dual, np.ascontiguousarray(sol.rho[full])


def pair_decisions(batch: Batch, sol: Solution, p):
    """The held-out decision values of pair p in the order of ``batch.held[p]``: the solved folds' ``dec``, the constants elsewhere."""
    out = batch.const[p].copy()
    n = len(batch.held[p])
    chunks = [(f * n // N_FOLDS, (f + 1) * n // N_FOLDS) for f in range(N_FOLDS)]
    for q in np.flatnonzero((batch.pair == p) & (batch.kind >= 0)):
        b, e = chunks[int(batch.kind[q])]
        pr = batch.problems[q]
        out[b:e] = sol.dec[pr["eval0"]: pr["eval0"] + pr["n_eval"]]
    return out


def fit_arrays(K, y_idx, k, c_of_class, eps, max_iter, random_state, solve):
    """(n_support, support, dual_coef, rho, probA, probB, fit_info) of the members' kernel matrix ``K`` and class numbers."""
    batch = build_batch(y_idx, k, c_of_class, random_state)
    check_batch(batch)
    n = batch.problems["n_pos"].astype(np.int64) + batch.problems["n_neg"]
    sol = solve(K, batch, eps, effective_max_iter(max_iter, n.max()))
    n_support, support, dual, rho = assemble(y_idx, k, batch, sol)
    AB = [sigmoid_train(pair_decisions(batch, sol, p), batch.held_y[p]) for p in range(len(batch.pairs))]
    info = {"pairs": list(batch.pairs), "pair": batch.pair.copy(), "fold": batch.kind.copy(), "rows": n, "n_iter": sol.n_iter.copy(),
            "state": sol.state.copy()}
    return n_support, support, dual, rho, np.array([a for a, _ in AB]), np.array([b for _, b in AB]), info
