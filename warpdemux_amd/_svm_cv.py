"""Cross-validated probabilities of a DTW kernel machine: the plan of ONE batched solve that fits every outer fold (and, on
request, the full data) on one resident kernel matrix, and the host work behind it.  Builds on `_svm_fit`; nothing here touches a
device -- the solver is an argument, so the tests run the plan on the NumPy restatement of the solver's rule.

THE OUTER FOLDS are this engine's own.  A class needs at least ``cv`` members (2 <= cv <= 10).  Class c's member rows in
ascending order are permuted with ``np.random.default_rng([random_state, c, c])`` -- `_svm_fit` seeds its pairs' inner folds
with ``[random_state, i, j]``, i < j, so the two families cannot collide -- and fold f holds out entries
``f * n_c // cv .. (f + 1) * n_c // cv`` of that permutation.  ``H_f`` is the union of those over the classes, ascending;
``T_f`` the other rows, ascending.  Every fold's training part therefore holds every class.

FOLD f's PROBLEMS are exactly ``_svm_fit.build_batch(y_idx[T_f], k, C * weights_f, random_state)`` -- ``weights_f`` the class
weights computed on ``T_f`` -- with its row numbers mapped through ``T_f``, but each pair's FULL problem names all of ``H_f``
(of whatever class) as its evaluation rows: its decision values on the held-out rows come out of the same launch.  Fold f's
model is therefore, bit for bit, what ``_svm_fit.fit_arrays`` returns on ``K[T_f][:, T_f]``.

The batches of all folds are concatenated, the full data's own batch behind them when ``with_full`` is set, and solved in one
wdx_svm_solve_device launch.  Afterwards the host runs `_svm_fit.sigmoid_train` per (fold, pair) on the inner folds' held-out
decision values: ``probA`` / ``probB`` per fold, which wdx_svm_cv_couple_device turns, with the full problems' decision values on
``H_f``, into the out-of-fold probabilities.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import numpy as np

from . import _svm_fit

MIN_CV, MAX_CV = 2, 10


class CvPlan(NamedTuple):
    """``batch``: the concatenated problems (``rows`` / ``eval_rows`` in member-row numbers: what the solver takes).  Part g is
    fold g for g < cv and the full data for g == cv (``with_full``); ``part_of[q]`` is problem q's part, ``first[g]`` its first
    problem (``first[-1]``: the number of problems), ``sub[g]`` its `_svm_fit.Batch` in the part's OWN row numbers (what
    ``build_batch`` returned), ``weights[g]`` its class weights.  ``train[f]`` / ``held[f]``: T_f / H_f."""

    batch: _svm_fit.Batch
    k: int
    cv: int
    with_full: bool
    fold_of_row: np.ndarray
    train: List[np.ndarray]
    held: List[np.ndarray]
    part_of: np.ndarray
    first: List[int]
    sub: List[_svm_fit.Batch]
    rows_local: np.ndarray
    weights: List[np.ndarray]


def check_cv(cv, counts):
    if not isinstance(cv, (int, np.integer)) or not MIN_CV <= cv <= MAX_CV:
        raise ValueError(f"cv must be an integer in {MIN_CV} .. {MAX_CV}, not {cv!r}")
    counts = np.asarray(counts)
    if counts.min() < cv:
        c = int(np.argmin(counts))
        raise ValueError(f"class {c} has {int(counts[c])} members, fewer than cv = {cv}")


def outer_folds(y_idx, k, cv=5, random_state=0):
    """(fold_of_row int32 (m,), [T_f], [H_f]) by the stated rule."""
    y_idx = np.asarray(y_idx)
    check_cv(cv, np.bincount(y_idx, minlength=k)[:k])
    fold = np.full(len(y_idx), -1, dtype=np.int32)
    for c in range(k):
        perm = np.random.default_rng([int(random_state), c, c]).permutation(np.flatnonzero(y_idx == c))
        n = len(perm)
        for f in range(cv):
            fold[perm[f * n // cv: (f + 1) * n // cv]] = f
    held = [np.flatnonzero(fold == f).astype(np.int32) for f in range(cv)]
    train = [np.flatnonzero(fold != f).astype(np.int32) for f in range(cv)]
    return fold, train, held


def plan(y_idx, k, C, class_weight, classes, random_state=0, cv=5, with_full=False) -> CvPlan:
    """``classes``: the k class labels (for a ``class_weight`` dict); ``C``: the SVC's C."""
    y_idx = np.asarray(y_idx)
    fold, train, held = outer_folds(y_idx, k, cv, random_state)
    problems, rows, rows_local, evals, kind, pair_of, part_of, first, sub, weights = [], [], [], [], [], [], [], [], [], []
    n_rows = n_eval = 0
    parts = [(train[f], held[f]) for f in range(cv)]
    if with_full:
        parts.append((np.arange(len(y_idx), dtype=np.int32), np.zeros(0, np.int32)))
    pairs = None
    for g, (T, H) in enumerate(parts):
        w = _svm_fit.class_weights(class_weight, classes, y_idx[T])
        b = _svm_fit.build_batch(y_idx[T], k, C * w, random_state)
        pairs = b.pairs
        first.append(len(problems))
        sub.append(b)
        weights.append(w)
        for q, pr in enumerate(b.problems):
            nr = int(pr["n_pos"]) + int(pr["n_neg"])
            local = b.rows[pr["row0"]: pr["row0"] + nr]
            ev = H if b.kind[q] == -1 else T[b.eval_rows[pr["eval0"]: pr["eval0"] + pr["n_eval"]]]
            problems.append((n_rows, n_eval, int(pr["n_pos"]), int(pr["n_neg"]), len(ev), 0, float(pr["c_pos"]), float(pr["c_neg"])))
            rows_local.append(local)
            rows.append(T[local])
            evals.append(ev)
            n_rows += nr
            n_eval += len(ev)
            kind.append(int(b.kind[q]))
            pair_of.append(int(b.pair[q]))
            part_of.append(g)
    first.append(len(problems))
    cat = lambda parts_: np.ascontiguousarray(np.concatenate(parts_) if parts_ else np.zeros(0), dtype=np.int32)   # noqa: E731
    batch = _svm_fit.Batch(np.array(problems, dtype=_svm_fit.PROBLEM_DTYPE), cat(rows), cat(evals), pairs, np.array(kind, np.int32),
                           np.array(pair_of, np.int32), [], [], [])
    return CvPlan(batch, int(k), int(cv), bool(with_full), fold, train, held, np.array(part_of, np.int32), first, sub, cat(rows_local), weights)


def largest_problem(p: CvPlan) -> int:
    return int((p.batch.problems["n_pos"].astype(np.int64) + p.batch.problems["n_neg"]).max())


def part_batch(p: CvPlan, g) -> _svm_fit.Batch:
    """Part g's problems as a `_svm_fit.Batch` whose offsets point into the WHOLE solution and whose rows are the part's own
    numbers: what `_svm_fit.assemble` and `_svm_fit.pair_decisions` take together with the whole solution's ``alpha`` and ``dec``."""
    sl = slice(p.first[g], p.first[g + 1])
    b = p.sub[g]
    return _svm_fit.Batch(p.batch.problems[sl], p.rows_local, p.batch.eval_rows, b.pairs, p.batch.kind[sl], p.batch.pair[sl], b.held, b.held_y,
                          b.const)


def part_arrays(p: CvPlan, g, y_idx, sol: _svm_fit.Solution):
    """(n_support, support, dual_coef, rho, probA, probB) of part g -- `_svm_fit.fit_arrays` behind the solve, on the part's rows."""
    y_idx = np.asarray(y_idx)
    T = p.train[g] if g < p.cv else np.arange(len(y_idx))
    b = part_batch(p, g)
    sl = slice(p.first[g], p.first[g + 1])   # (alpha and dec keep the whole solution's offsets; the per-problem values are the part's)
    sol = _svm_fit.Solution(sol.alpha, sol.rho[sl], sol.n_iter[sl], sol.state[sl], sol.dec)
    n_support, support, dual, rho = _svm_fit.assemble(y_idx[T], p.k, b, sol)
    AB = [_svm_fit.sigmoid_train(_svm_fit.pair_decisions(b, sol, q), b.held_y[q]) for q in range(len(b.pairs))]
    return n_support, support, dual, rho, np.array([a for a, _ in AB]), np.array([b_ for _, b_ in AB])


def couple_tables(p: CvPlan, probA, probB):
    """The host tables of wdx_svm_cv_couple_device: (dec_off int64 (cv, pairs): where each (fold, pair)'s full problem keeps its
    decision values on H_f; A, B float64 (cv, pairs); held int32: H_0 | H_1 | ..; held_off int64 (cv + 1,))."""
    n_pairs = len(p.batch.pairs)
    off = np.zeros((p.cv, n_pairs), np.int64)
    for f in range(p.cv):
        for q in range(p.first[f], p.first[f + 1]):
            if p.batch.kind[q] == -1:
                off[f, p.batch.pair[q]] = p.batch.problems[q]["eval0"]
    held_off = np.zeros(p.cv + 1, np.int64)
    held_off[1:] = np.cumsum([len(h) for h in p.held])
    A = np.ascontiguousarray(np.asarray(probA, dtype=np.float64).reshape(p.cv, n_pairs))
    B = np.ascontiguousarray(np.asarray(probB, dtype=np.float64).reshape(p.cv, n_pairs))
    return off, A, B, np.ascontiguousarray(np.concatenate(p.held), dtype=np.int32), held_off


def fit_info(p: CvPlan, sol: _svm_fit.Solution):
    return {"pairs": list(p.batch.pairs), "pair": p.batch.pair.copy(), "fold": p.batch.kind.copy(), "part": p.part_of.copy(),
            "rows": p.batch.problems["n_pos"].astype(np.int64) + p.batch.problems["n_neg"], "n_iter": np.asarray(sol.n_iter).copy(),
            "state": np.asarray(sol.state).copy()}


def solve_parts(K, y_idx, k, C, class_weight, classes, eps, max_iter, random_state, cv, with_full, solve, p: Optional[CvPlan] = None):
    """(plan, solution, [part_arrays per part]) with ``solve(K, batch, eps, cap) -> _svm_fit.Solution``: the whole host route,
    for the tests and for callers without a resident matrix."""
    p = p or plan(y_idx, k, C, class_weight, classes, random_state, cv, with_full)
    _svm_fit.check_batch(p.batch)
    sol = solve(K, p.batch, eps, _svm_fit.effective_max_iter(max_iter, largest_problem(p)))
    return p, sol, [part_arrays(p, g, y_idx, sol) for g in range(len(p.sub))]
