"""The SMO rule of the device solver and the host code around it, without a GPU.

1. tests/helpers/svm_fit_rule.py (the NumPy restatement the kernel is held to bit for bit) against scikit-learn's libsvm on the
   same kernel matrix: K = exp(-D), D the Euclidean distance of seeded rows (window-1 DTW: K is positive semi-definite), 600 rows
   of 4 classes and 1 500 rows of 6, noise of 0.9 / 1.1 sigma around the class templates so that every row is a support vector,
   ``SVC(C=1, class_weight="balanced", tol=1e-3)`` -- the recipe of the shipped models.
     KKT        kkt.worst(kkt.kkt_residuals(...)) <= kkt.EPS_LIBSVM: the stopping rule gmax - gmin < eps with rho inside
                [gmin, gmax] implies it.
     objective  per pair |objective - scikit-learn's| <= eps * sum of C_s: for a positive semi-definite K a point whose gap is
                below eps lies within eps * sum C_s of the optimum (the duality gap of the box-constrained dual is at most
                sum_s C_s * violation_s), and both solutions are such points.  The observed differences are printed.
2. `_svm_fit`: the batch (pairs, folds, constant folds), `sigmoid_train` against a hand-worked case, `assemble` against
   scikit-learn's own layout, `class_weight` on the libsvm path of `DTW_SVM.fit`, and every refusal before any device work."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import kkt  # noqa: E402
from helpers import svm_fit_rule as rule  # noqa: E402
from warpdemux_amd import _lib, _svm_fit  # noqa: E402
from warpdemux_amd.models import DTW_SVM  # noqa: E402

CASES = {"600x4": (600, 4, 0.9), "1500x6": (1500, 6, 1.1)}
EPS = kkt.EPS_LIBSVM


@functools.lru_cache(maxsize=None)
def _case(name):
    """(D float32, K float32, y, the fitted SVC, the restatement's Solution of the full problems and their Batch)"""
    from sklearn.svm import SVC

    n, k, noise = CASES[name]
    rng = np.random.default_rng(3 + n)
    T = rng.normal(size=(k, 25))
    y = np.sort(rng.integers(0, k, n))
    X = T[y] + noise * rng.normal(size=(n, 25))
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    K = np.exp(-D)
    svc = SVC(kernel="precomputed", C=1.0, class_weight="balanced", tol=EPS).fit(K, y)
    w = _svm_fit.class_weights("balanced", np.arange(k), y)
    batch = _svm_fit.build_batch(y, k, 1.0 * w, folds=False)
    sol = rule.solve_batch(K, batch, EPS, rule.default_max_iter(n))
    for a in (D, K, y):
        a.setflags(write=False)
    return D, K, y, svc, batch, sol, w


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_meets_the_kkt_conditions_like_libsvm(name):
    D, K, y, svc, batch, sol, w = _case(name)
    k = CASES[name][1]
    assert np.allclose(w, svc.class_weight_)
    assert svc.support_.size == len(y), "the generator was built so that every row is a support vector"
    assert (sol.state == 0).all()
    n_support, support, dual, rho = _svm_fit.assemble(y, k, batch, sol)
    assert np.array_equal(support, np.arange(len(y))) and np.array_equal(n_support, np.bincount(y)), "every row a support vector here too"
    mine = kkt.worst(kkt.kkt_residuals(D, n_support, dual, -rho, w))
    theirs = kkt.worst(kkt.kkt_residuals(D, svc.n_support_, svc._dual_coef_, svc._intercept_, svc.class_weight_))
    per_problem = max(rule.kkt_worst(K, batch.rows[p["row0"]:p["row0"] + p["n_pos"] + p["n_neg"]], p["n_pos"], p["c_pos"], p["c_neg"],
                                     sol.alpha[p["row0"]:p["row0"] + p["n_pos"] + p["n_neg"]], sol.rho[q]) for q, p in enumerate(batch.problems))
    print(name, "worst KKT residual: restatement", mine, "scikit-learn", theirs, "all-rows helper", per_problem, "iterations", sol.n_iter.tolist())
    assert theirs <= EPS, "scikit-learn's own solution misses the bound: the generator is wrong"
    assert mine <= EPS and per_problem <= EPS


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reaches_libsvms_objective(name):
    D, K, y, svc, batch, sol, w = _case(name)
    k = CASES[name][1]
    worst_ratio, worst = 0.0, 0.0
    for q, ((i, j), p) in enumerate(zip(batch.pairs, batch.problems)):
        rows = batch.rows[p["row0"]:p["row0"] + p["n_pos"] + p["n_neg"]]
        mine = rule.objective(K, rows, p["n_pos"], sol.alpha[p["row0"]:p["row0"] + len(rows)])
        coef = np.concatenate([svc._dual_coef_[j - 1, rows[:p["n_pos"]]], svc._dual_coef_[i, rows[p["n_pos"]:]]])   # every row is a support vector
        theirs = rule.objective(K, rows, p["n_pos"], np.abs(coef))
        bound = EPS * (p["n_pos"] * p["c_pos"] + p["n_neg"] * p["c_neg"])
        print(name, "pair", (i, j), "objective", mine, "scikit-learn", theirs, "difference %.3e" % (mine - theirs), "bound %.3f" % bound)
        assert abs(mine - theirs) <= bound
        worst, worst_ratio = max(worst, abs(mine - theirs)), max(worst_ratio, abs(mine - theirs) / bound)
    print(name, "largest |difference|", worst, "largest share of its bound", worst_ratio)


# ---- the batch ----------------------------------------------------------------------------------------------------------------------

def test_batch_holds_every_pair_and_five_folds_by_the_stated_rule():
    rng = np.random.default_rng(0)
    y = rng.integers(0, 3, 50)
    c = np.array([1.0, 2.0, 0.5])
    b = _svm_fit.build_batch(y, 3, c, random_state=7)
    assert b.pairs == [(0, 1), (0, 2), (1, 2)] and len(b.problems) == 18
    assert b.kind.tolist() == [-1, 0, 1, 2, 3, 4] * 3 and b.pair.tolist() == [0] * 6 + [1] * 6 + [2] * 6
    at_r = at_e = 0
    for q, p in enumerate(b.problems):
        i, j = b.pairs[b.pair[q]]
        assert p["row0"] == at_r and p["eval0"] == at_e and p["c_pos"] == c[i] and p["c_neg"] == c[j]
        rows = b.rows[at_r:at_r + p["n_pos"] + p["n_neg"]]
        ev = b.eval_rows[at_e:at_e + p["n_eval"]]
        assert (y[rows[:p["n_pos"]]] == i).all() and (y[rows[p["n_pos"]:]] == j).all()
        assert (np.diff(rows[:p["n_pos"]]) > 0).all() and (np.diff(rows[p["n_pos"]:]) > 0).all(), "ascending within a side"
        members = np.flatnonzero((y == i) | (y == j))
        if b.kind[q] == -1:
            assert np.array_equal(np.sort(rows), members) and len(ev) == 0
        else:
            perm = np.random.default_rng([7, i, j]).permutation(members)
            f, n = int(b.kind[q]), len(members)
            assert np.array_equal(ev, perm[f * n // 5:(f + 1) * n // 5]), "fold f holds out the f-th contiguous chunk of the permutation"
            assert np.array_equal(np.sort(np.concatenate([rows, ev])), members) and not set(rows) & set(ev)
        at_r, at_e = at_r + len(rows), at_e + len(ev)
    assert at_r == len(b.rows) and at_e == len(b.eval_rows)
    for p_, (i, j) in enumerate(b.pairs):
        assert np.array_equal(b.held[p_], np.random.default_rng([7, i, j]).permutation(np.flatnonzero((y == i) | (y == j))))
        assert np.array_equal(b.held_y[p_], np.where(y[b.held[p_]] == i, 1.0, -1.0)) and np.isnan(b.const[p_]).all()
    other = _svm_fit.build_batch(y, 3, c, random_state=8)
    assert not np.array_equal(other.eval_rows, b.eval_rows), "the seed moves the folds"


def test_a_fold_without_a_side_takes_libsvms_constant_and_is_not_solved():
    y = np.array([0, 1, 1, 1, 1, 1, 1, 1, 1, 1])          # class 0 has one row: the fold that holds it out has no positive side
    b = _svm_fit.build_batch(y, 2, np.ones(2), random_state=0)
    perm = b.held[0]
    f_out = int(np.flatnonzero(perm == 0)[0]) * 5 // 10
    assert sorted(b.kind.tolist()) == sorted([-1] + [f for f in range(5) if f != f_out])
    want = np.full(10, np.nan)
    want[f_out * 2:f_out * 2 + 2] = -1.0
    assert np.array_equal(np.isnan(b.const[0]), np.isnan(want)) and np.array_equal(b.const[0][~np.isnan(want)], [-1.0, -1.0])
    two = _svm_fit.build_batch(np.array([0, 1]), 2, np.ones(2), random_state=0)   # two rows: three empty chunks, two one-sided folds
    assert two.kind.tolist() == [-1]
    c = two.const[0]
    assert np.array_equal(c, np.where(two.held_y[0] > 0, -1.0, 1.0)), "holding out the only row of a side leaves the other side"
    sol = rule.solve_batch(np.eye(2, dtype=np.float32), two, 1e-3, 100)
    assert np.array_equal(_svm_fit.pair_decisions(two, sol, 0), c)


def test_sigmoid_train_on_a_hand_worked_case():
    """Two points, dec = +1 (y = +1) and -1 (y = -1): the targets are 2/3 and 1/3 and B = log(2/2) = 0, so by symmetry B stays 0
    and A solves 1 / (1 + exp(A)) = 2/3: A = -log 2.  The regularised Newton iteration gets there to its own 1e-5 gradient test."""
    A, B = _svm_fit.sigmoid_train(np.array([1.0, -1.0]), np.array([1.0, -1.0]))
    assert abs(A + np.log(2.0)) < 1e-4 and abs(B) < 1e-9, (A, B)
    # one-sided labels: B starts at log(1 / (n + 1)) and the fit must stay finite
    A, B = _svm_fit.sigmoid_train(np.array([0.5, 1.5, 2.5]), np.array([1.0, 1.0, 1.0]))
    assert np.isfinite(A) and np.isfinite(B)
    # against the closed form of a separable two-level case: dec = +-d, n each: p(+d) = (n + 1) / (n + 2)
    d, n = 2.0, 7
    A, B = _svm_fit.sigmoid_train(np.r_[np.full(n, d), np.full(n, -d)], np.r_[np.ones(n), -np.ones(n)])
    assert abs(B) < 1e-8 and abs(1.0 / (1.0 + np.exp(A * d)) - (n + 1.0) / (n + 2.0)) < 1e-5


def test_assemble_gives_libsvms_layout():
    """on a case where only some rows are support vectors: the restatement's alpha through `assemble` against the SVC's own arrays
    -- the same support rows in the same order, and decision values within the two stopping tolerances of each other"""
    from sklearn.svm import SVC

    rng = np.random.default_rng(5)
    k, n = 3, 240
    y = rng.integers(0, k, n)                      # unsorted labels: the grouping by class is `assemble`'s
    X = 4.0 * rng.normal(size=(k, 6))[y] + rng.normal(size=(n, 6))
    K = np.exp(-0.2 * np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))).astype(np.float32)
    svc = SVC(kernel="precomputed", C=1.0, tol=1e-5).fit(K, y)
    batch = _svm_fit.build_batch(y, k, np.ones(k), folds=False)
    sol = rule.solve_batch(K, batch, 1e-5, 10_000_000)
    n_support, support, dual, rho = _svm_fit.assemble(y, k, batch, sol)
    assert support.dtype == np.int32 and dual.shape == (k - 1, len(support)) and n_support.sum() == len(support) < n
    for c in range(k):
        rows = support[n_support[:c].sum():n_support[:c + 1].sum()]
        assert (y[rows] == c).all() and (np.diff(rows) > 0).all()
    assert np.array_equal(support, svc.support_), "the same support rows, grouped and ordered as libsvm does"
    assert np.abs(dual - svc._dual_coef_).max() < 5e-3 and np.abs(-rho - svc._intercept_).max() < 5e-4
    # pair (i, j): class i's coefficients are positive in row j - 1, class j's negative in row i
    start = np.r_[0, np.cumsum(n_support)]
    for (i, j) in batch.pairs:
        assert (dual[j - 1, start[i]:start[i + 1]] >= 0).all() and (dual[i, start[j]:start[j + 1]] <= 0).all()


def test_fit_arrays_end_to_end_on_the_restatement():
    D, K, y, svc, _, _, w = _case("600x4")
    n_support, support, dual, rho, probA, probB, info = _svm_fit.fit_arrays(K, y, 4, 1.0 * w, EPS, -1, 0, rule.solve_batch)
    assert probA.shape == probB.shape == rho.shape == (6,) and (probA < 0).all(), "a larger decision value means class i"
    assert len(info["state"]) == 36 and (info["state"] == 0).all() and info["fold"].tolist() == [-1, 0, 1, 2, 3, 4] * 6
    assert kkt.worst(kkt.kkt_residuals(D, n_support, dual, -rho, w)) <= EPS


# ---- DTW_SVM.fit: the libsvm path's new arguments, and the refusals --------------------------------------------------------------------

def _rows(n=120, k=3, L=8, seed=2):
    rng = np.random.default_rng(seed)
    y = np.r_[np.zeros(n // 2, int), np.ones(n // 3, int), np.full(n - n // 2 - n // 3, 2)]
    X = 3.0 * rng.normal(size=(k, L))[y] + rng.normal(size=(n, L))
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    return X, y * 5 + 1, D


def test_class_weight_reaches_the_svc_on_the_libsvm_path_and_the_defaults_are_unchanged():
    from sklearn.svm import SVC

    X, y, D = _rows()
    K = np.exp(-1.0 * np.power(D, 1))
    plain = DTW_SVM.fit(X, y, 15, 0.1, distances=D)
    want = SVC(kernel="precomputed", probability=True, C=1.0, random_state=0).fit(K, y)
    assert np.array_equal(plain._dual_coef, want._dual_coef_) and np.array_equal(plain._probA, want._probA)
    for cw in ("balanced", {1: 2.0, 11: 0.5}):
        got = DTW_SVM.fit(X, y, 15, 0.1, distances=D, class_weight=cw, tol=1e-4, max_iter=5000)
        want = SVC(kernel="precomputed", probability=True, C=1.0, random_state=0, class_weight=cw, tol=1e-4, max_iter=5000).fit(K, y)
        assert np.array_equal(got._dual_coef, want._dual_coef_) and np.array_equal(got._rho, -want._intercept_)
        assert np.array_equal(got._probA, want._probA)
        assert got._dual_coef.shape != plain._dual_coef.shape or not np.array_equal(got._dual_coef, plain._dual_coef), "the weights changed nothing"
    assert np.allclose(_svm_fit.class_weights("balanced", np.array([1, 6, 11]), (y - 1) // 5), 120 / (3 * np.bincount((y - 1) // 5)))
    assert np.array_equal(_svm_fit.class_weights({1: 2.0, 11: 0.5}, np.array([1, 6, 11]), (y - 1) // 5), [2.0, 1.0, 0.5])


def test_every_refusal_comes_before_any_device_work():
    """`distances` is not given, so a fit that got past its checks would ask the device for the matrix: each of these raises its
    own error first, GPU or not"""
    X, y, D = _rows()
    for kw, exc, match in (
            (dict(solver="gpu"), ValueError, 'solver must be "libsvm" or "device"'),
            (dict(solver="device", class_weight="even"), ValueError, "class_weight must be None"),
            (dict(solver="libsvm", class_weight="even"), ValueError, "class_weight must be None"),
            (dict(solver="device", class_weight={2: 1.0}), ValueError, "not among the members' labels"),
            (dict(solver="device", class_weight={1: -1.0}), ValueError, "positive and finite"),
            (dict(solver="device", tol=0.0), ValueError, "tol must be positive"),
            (dict(solver="device", C=float("inf")), ValueError, "C must be positive"),
            (dict(solver="device", max_iter=-2), ValueError, "max_iter must be -1 or"),
            (dict(solver="device", max_iter=2.5), ValueError, "max_iter must be -1 or"),
            (dict(solver="device", random_state=None), ValueError, "non-negative integer random_state"),
            (dict(solver="device", random_state=-1), ValueError, "non-negative integer random_state")):
        with pytest.raises(exc, match=match):
            DTW_SVM.fit(X, y, 15, 0.1, **kw)
    big = _lib.SVM_FIT_MAX_ROWS // 2 + 1
    with pytest.raises(NotImplementedError, match="more than WDX_SVM_FIT_MAX_ROWS = 16384"):
        DTW_SVM.fit(np.zeros((2 * big + 3, 4)), np.r_[np.zeros(big, int), np.ones(big, int), [2, 2, 2]], 15, 0.1, solver="device")
    with pytest.raises(NotImplementedError, match="more than WDX_SVM_FIT_MAX_ROWS"):
        _svm_fit.check_batch(_svm_fit.build_batch(np.r_[np.zeros(big, int), np.ones(big, int)], 2, np.ones(2), folds=False))
    assert _svm_fit.effective_max_iter(-1, 16384) == 10_000_000 and _svm_fit.effective_max_iter(-1, 200_000) == 20_000_000
    assert _svm_fit.effective_max_iter(0, 5) == 0
