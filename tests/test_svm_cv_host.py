"""The cross-validation plan (warpdemux_amd/_svm_cv.py) without a device: the outer folds by their stated rule, a fold's problems
against `_svm_fit.build_batch` on its training rows, and -- with the NumPy solver of tests/helpers/svm_fit_rule.py -- a fold's
model arrays against `_svm_fit.fit_arrays` on ``K[T_f][:, T_f]``, bit for bit.  Shape: m = 120, k = 4, cv = 5."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import svm_fit_rule as rule  # noqa: E402
from warpdemux_amd import _svm_cv, _svm_fit  # noqa: E402

M, K_CLASSES, CV, SEED = 120, 4, 5, 3


@functools.lru_cache(maxsize=None)
def _data():
    rng = np.random.default_rng(11)
    y = rng.permutation(np.repeat(np.arange(K_CLASSES), [40, 35, 25, 20]))
    X = rng.normal(size=(M, 6)) + 1.2 * np.eye(K_CLASSES, 6)[y]
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    return np.exp(-0.5 * D).astype(np.float32), y


def test_outer_folds_partition_the_members_by_the_stated_seeds():
    _, y = _data()
    fold, train, held = _svm_cv.outer_folds(y, K_CLASSES, CV, SEED)
    assert fold.dtype == np.int32 and set(fold.tolist()) == set(range(CV))
    assert np.array_equal(np.sort(np.concatenate(held)), np.arange(M))
    for f in range(CV):
        assert np.array_equal(np.sort(np.concatenate([train[f], held[f]])), np.arange(M))
        assert (np.diff(train[f]) > 0).all() and (np.diff(held[f]) > 0).all()
        assert set(y[train[f]].tolist()) == set(range(K_CLASSES))            # every training part holds every class
    for c in range(K_CLASSES):
        perm = np.random.default_rng([SEED, c, c]).permutation(np.flatnonzero(y == c))
        n = len(perm)
        for f in range(CV):
            assert set(perm[f * n // CV: (f + 1) * n // CV].tolist()) == set(held[f][y[held[f]] == c].tolist())
    other = _svm_cv.outer_folds(y, K_CLASSES, CV, SEED + 1)[0]
    assert not np.array_equal(other, fold)


def test_cv_beyond_a_class_is_refused():
    _, y = _data()
    for cv in (1, 11, 2.0, None):
        with pytest.raises(ValueError):
            _svm_cv.outer_folds(y, K_CLASSES, cv, 0)
    y2 = y.copy()
    y2[np.flatnonzero(y2 == 3)[4:]] = 0                                       # class 3 keeps four members
    with pytest.raises(ValueError, match="class 3 has 4 members"):
        _svm_cv.plan(y2, K_CLASSES, 1.0, None, np.arange(K_CLASSES), 0, 5)
    _svm_cv.plan(y2, K_CLASSES, 1.0, None, np.arange(K_CLASSES), 0, 4)


@pytest.mark.parametrize("class_weight", [None, "balanced"])
def test_fold_batch_is_build_batch_on_the_training_rows(class_weight):
    _, y = _data()
    C = 2.0
    p = _svm_cv.plan(y, K_CLASSES, C, class_weight, np.arange(K_CLASSES), SEED, CV, with_full=True)
    n_pairs = K_CLASSES * (K_CLASSES - 1) // 2
    assert len(p.batch.problems) == (CV + 1) * n_pairs * (1 + _svm_fit.N_FOLDS) == p.first[-1] and p.first[1] == 36
    parts = [(p.train[f], p.held[f]) for f in range(CV)] + [(np.arange(M), np.zeros(0, np.int32))]
    for g, (T, H) in enumerate(parts):
        w = _svm_fit.class_weights(class_weight, np.arange(K_CLASSES), y[T])
        b = _svm_fit.build_batch(y[T], K_CLASSES, C * w, SEED)
        assert len(b.problems) == p.first[g + 1] - p.first[g]
        for q, pr in enumerate(b.problems):
            got = p.batch.problems[p.first[g] + q]
            for name in ("n_pos", "n_neg", "c_pos", "c_neg"):
                assert got[name] == pr[name]
            nr = int(pr["n_pos"]) + int(pr["n_neg"])
            assert np.array_equal(p.batch.rows[got["row0"]: got["row0"] + nr], T[b.rows[pr["row0"]: pr["row0"] + nr]])
            ev = p.batch.eval_rows[got["eval0"]: got["eval0"] + got["n_eval"]]
            if b.kind[q] == -1:
                assert np.array_equal(ev, H)                                   # the full problem evaluates ALL held-out rows
            else:
                assert np.array_equal(ev, T[b.eval_rows[pr["eval0"]: pr["eval0"] + pr["n_eval"]]])
            assert p.batch.kind[p.first[g] + q] == b.kind[q] and p.batch.pair[p.first[g] + q] == b.pair[q] and p.part_of[p.first[g] + q] == g
    assert p.batch.problems["row0"][-1] + p.batch.problems["n_pos"][-1] + p.batch.problems["n_neg"][-1] == len(p.batch.rows)
    assert p.batch.problems["eval0"][-1] + p.batch.problems["n_eval"][-1] == len(p.batch.eval_rows)


def test_fold_models_equal_fit_arrays_on_the_training_block():
    K, y = _data()
    C, eps = 1.0, 1e-3
    p, sol, parts = _svm_cv.solve_parts(K, y, K_CLASSES, C, "balanced", np.arange(K_CLASSES), eps, -1, SEED, CV, True, rule.solve_batch)
    assert (sol.state == 0).all()
    for g in range(CV + 1):
        T = p.train[g] if g < CV else np.arange(M)
        w = _svm_fit.class_weights("balanced", np.arange(K_CLASSES), y[T])
        want = _svm_fit.fit_arrays(np.ascontiguousarray(K[T][:, T]), y[T], K_CLASSES, C * w, eps, -1, SEED, rule.solve_batch)
        for a, b in zip(parts[g], want[:6]):
            assert np.array_equal(a, b), g
    # the full problems' decision values on the held-out rows: the fold model's own decision function on K[H_f][:, T_f]
    off, A, B, held, held_off = _svm_cv.couple_tables(p, [a[4] for a in parts[:CV]], [a[5] for a in parts[:CV]])
    assert held_off.tolist() == np.concatenate([[0], np.cumsum([len(h) for h in p.held])]).tolist() and np.array_equal(held, np.concatenate(p.held))
    for f in (0, CV - 1):
        n_support, support, dual, rho = parts[f][:4]
        T, H = p.train[f], p.held[f]
        start = np.concatenate([[0], np.cumsum(n_support)])
        for q, (i, j) in enumerate(p.batch.pairs):
            kv = K[H][:, T[support]].astype(np.float64)
            si, sj = slice(start[i], start[i + 1]), slice(start[j], start[j + 1])
            dec = kv[:, si] @ dual[j - 1, si] + kv[:, sj] @ dual[i, sj] - rho[q]
            np.testing.assert_allclose(sol.dec[off[f, q]: off[f, q] + len(H)], dec, rtol=0, atol=1e-12)
    info = _svm_cv.fit_info(p, sol)
    assert (info["part"] == p.part_of).all() and len(info["state"]) == len(p.batch.problems)
