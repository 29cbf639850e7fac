"""The training rule of the device Fpt_Boost trainer and the host code around it, without a GPU.

tests/helpers/boost_fit_rule.py (the NumPy restatement of include/wdx.h's wdx_boost_fit_device rule) is held to its own claims:
1. ``exp_rule`` is within 2**-51 relative of ``np.exp`` in long double on [-700, 0] and is 0 below;
2. the borders rule on a constant column, an all-NaN column, a column with fewer unique values than B and a heavy-duplicates
   column -- and `_boost_fit.borders` (the package's own) gives the same borders;
3. the final scores of a fit equal ``boost_ref.raw_scores`` of the emitted model, ``array_equal``: the trainer and the existing tail
   agree to the last bit by construction;
4. the training log-loss after 20 trees is below that after 1 on a separable synthetic set;
5. the header's constants equal `_lib`'s;
6. every refusal `Fpt_Boost.fit` makes before any device work."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import boost_fit_rule as rule  # noqa: E402
from helpers import boost_ref  # noqa: E402
from warpdemux_amd import _boost_fit, _lib  # noqa: E402
from warpdemux_amd.models import Fpt_Boost  # noqa: E402


def test_exp_rule_against_long_double():
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-700, 0, 400_000), rng.uniform(-2, 0, 100_000), -np.logspace(-300, 2.8, 20_000),
                        np.array([0.0, -0.0, -700.0, -1e-320, -np.log(2) / 2, -np.log(2), -699.9999999])])
    x = x[x >= -700.0]
    got = rule.exp_rule(x).astype(np.longdouble)
    want = np.exp(x.astype(np.longdouble))
    rel = np.abs(got - want) / want
    own = np.abs(np.exp(x).astype(np.longdouble) - want) / want
    print(f"exp_rule: max relative error {float(rel.max()):.3g} (np.exp float64: {float(own.max()):.3g}); 2**-51 = {2.0 ** -51:.3g}")
    assert float(rel.max()) <= 2.0 ** -51
    assert rule.exp_rule(np.array([0.0]))[0] == 1.0
    below = np.array([-700.0000001, -701.0, -1e4, -1e300, -np.inf])
    assert np.array_equal(rule.exp_rule(below), np.zeros(5))


def test_exp_coefficients_are_made_by_division():
    c = 1.0
    for i in range(1, 14):
        c = c / i
        assert rule.EXP_COEF[i] == c
    assert len(rule.EXP_COEF) == 14
    assert rule.LN2_HI + rule.LN2_LO == np.log(2.0) and rule.LOG2E == 1.4426950408889634


BORDER_COLUMNS = {
    "constant": (np.full(50, 2.5), 8, np.zeros(0, np.float32)),
    "all NaN": (np.full(50, np.nan), 8, np.zeros(0, np.float32)),
    "constant with NaNs": (np.where(np.arange(50) % 3 == 0, np.nan, 1.0), 8, np.zeros(0, np.float32)),
    "fewer unique values than B": (np.array([3.0, 1.0, 2.0, 3.0, 1.0, np.nan, 5.0]), 8, np.array([1.0, 2.0, 3.0], np.float32)),
    "exactly B + 1 unique values": (np.arange(9.0), 8, np.arange(8.0).astype(np.float32)),
    # 90 zeros, then 1 .. 10: s[(j * 100) // 5] for j = 1 .. 4 = s[20], s[40], s[60], s[80] = 0
    "heavy duplicates": (np.concatenate([np.zeros(90), np.arange(1.0, 11.0)]), 4, np.array([0.0], np.float32)),
    # 10 values then 90 copies of the maximum: the picks equal to the maximum are dropped; s[20 ..] = 9 -> nothing is left
    "duplicates of the maximum": (np.concatenate([np.arange(9.0), np.full(91, 9.0)]), 4, np.zeros(0, np.float32)),
    # 0 .. 99, B = 3: s[25], s[50], s[75]
    "quantiles": (np.arange(100.0)[::-1].copy(), 3, np.array([25.0, 50.0, 75.0], np.float32)),
}


@pytest.mark.parametrize("name", sorted(BORDER_COLUMNS))
def test_borders_rule(name):
    col, B, want = BORDER_COLUMNS[name]
    got = rule.feature_borders(col.astype(np.float32), B)
    assert got.dtype == np.float32 and np.array_equal(got, want), (got, want)
    assert np.array_equal(_boost_fit.feature_borders(col, B), want)
    if len(got):   # ascending data values with a row on both sides of x > border
        vals = col[~np.isnan(col)].astype(np.float32)
        assert np.all(np.diff(got) > 0) and np.isin(got, vals).all()
        for b in got:
            assert (vals > b).any() and (vals <= b).any()
    assert len(got) <= B


def test_borders_of_a_matrix_agree_with_the_package():
    X, _ = rule.synthetic(700, 9, 3, seed=5)
    X[::7, 2] = np.nan
    X[:, 4] = 1.0
    X[:, 5] = np.round(X[:, 5])
    for B in (1, 5, 32, 255):
        a, b = rule.borders(X, B), _boost_fit.borders(X, B)
        assert all(np.array_equal(x, y) and x.dtype == y.dtype == np.float32 for x, y in zip(a, b))
        assert len(a[4]) == 0 and all(len(x) <= B for x in a)
        bins = rule.binarise(X, a)
        assert all(int(bins[f].max()) == len(a[f]) for f in range(9)) and bins[2][::7].max() == 0


@pytest.fixture(scope="module")
def separable():
    X, y = rule.synthetic(600, 10, 4, seed=11, noise=0.7)
    fit1, S1 = rule.fit(X, y, 4, 1, 4, 0.3, 3.0, 32)
    fit20, S20 = rule.fit(X, y, 4, 20, 4, 0.3, 3.0, 32)
    return X, y, fit1, S1, fit20, S20


def test_final_scores_equal_the_tail_formula(separable):
    X, y, _, _, fit20, S20 = separable
    m = fit20.model(X.shape[1])
    assert len(m.trees) == 20 and m.dim == m.k == 4
    assert np.array_equal(boost_ref.raw_scores(m, X), S20)
    leaf = boost_ref.leaf_indices(m, X)
    assert leaf.max() < 16 and len(np.unique(leaf[0])) > 1


def test_a_continued_fit_equals_one_fit(separable):
    X, y, _, _, fit20, S20 = separable
    a, Sa = rule.fit(X, y, 4, 12, 4, 0.3, 3.0, 32)
    b, Sb = rule.fit(X, y, 4, 8, 4, 0.3, 3.0, 32, scores=Sa)
    assert np.array_equal(Sb, S20)
    assert all(np.array_equal(p, q) for p, q in zip(a.leaf_values + b.leaf_values, fit20.leaf_values))


def test_log_loss_falls(separable):
    X, y, _, S1, _, S20 = separable
    l1, l20 = rule.logloss(S1, y), rule.logloss(S20, y)
    print(f"training log-loss: {l1:.4f} after 1 tree, {l20:.4f} after 20")
    assert l20 < l1 < np.log(4)


def test_ties_go_to_the_lower_feature_and_border():
    X, y = rule.synthetic(200, 4, 3, seed=2)
    X[:, 3] = X[:, 1]
    fit, _ = rule.fit(X, y, 3, 3, 3, 0.5, 1.0, 16)
    assert all(3 not in f for f in fit.split_feature)


def test_no_feature_with_a_border_is_refused():
    with pytest.raises(rule.Refused):
        rule.fit(np.ones((5, 3)), np.array([0, 1, 0, 1, 0]), 2, 1, 2, 0.3, 3.0, 8)
    with pytest.raises(rule.Refused):
        rule.fit(np.array([[1.0, np.nan]]), np.array([0]), 2, 1, 2, 0.3, 3.0, 8)   # one row has no border


def test_constants_agree_across_the_layers():
    hdr = open(os.path.join(ROOT, "include", "wdx.h")).read()

    def define(name):
        return re.search(r"#define\s+%s\s+(.+?)\s*(/\*|$)" % name, hdr, re.M).group(1)

    assert int(define("WDX_K_BOOST_FIT")) == _lib.K_BOOST_FIT == 17
    assert int(define("WDX_BOOST_FIT_MAX_DEPTH")) == _lib.BOOST_FIT_MAX_DEPTH == 8
    assert int(define("WDX_BOOST_FIT_MAX_BORDERS")) == _lib.BOOST_FIT_MAX_BORDERS == 255
    assert define("WDX_BOOST_FIT_MAX_ROWS") == "(1 << 24)" and _lib.BOOST_FIT_MAX_ROWS == 1 << 24
    assert define("WDX_BOOST_FIT_MAX_TREES") == "(1 << 20)" and _lib.BOOST_FIT_MAX_TREES == 1 << 20
    assert define("WDX_BOOST_FIT_MAX_WORKSPACE") == "((int64_t)4 << 30)" and _lib.BOOST_FIT_MAX_WORKSPACE == 4 << 30
    assert int(define("WDX_BOOST_FIT_GRAD_BITS")) == _lib.BOOST_FIT_GRAD_BITS == rule.GRAD_BITS == 20
    assert int(define("WDX_BOOST_FIT_ROWS")) == _lib.BOOST_FIT_ROWS and _lib.BOOST_FIT_ROWS << 20 < 1 << 31
    assert "wdx_boost_fit_device" in _lib.EXPORTS and "wdx_boost_fit" in _lib.EXPORTS
    assert not any(name.startswith("wdx_boost_fit") and name.endswith("_dev") for name in _lib.EXPORTS)
    import ctypes as C

    assert C.sizeof(_lib.BoostFitParamsC) == 4 * 6 + 8 * 2
    # the constants of exp_rule as the header states them
    for text, value in (("0x1.71547652b82fep+0", rule.LOG2E), ("0x1.62e42feep-1", rule.LN2_HI), ("0x1.a39ef35793c76p-33", rule.LN2_LO)):
        assert text in hdr and float.fromhex(text) == value
    plan = open(os.path.join(ROOT, "warpdemux_amd", "csrc", "wdx_boost_fit_plan.h")).read()
    assert "kBoostFitExpDegree = 13" in plan and rule.EXP_DEGREE == 13


REFUSALS = {
    "X not 2-d": (dict(X=np.zeros(5)), ValueError, "X must be"),
    "y shape": (dict(y=np.zeros(3, np.int64)), ValueError, "one label per row"),
    "y dtype": (dict(y=np.zeros(40)), ValueError, "integer dtype"),
    "one class": (dict(y=np.zeros(40, np.int64)), ValueError, "at least two classes"),
    "17 classes": (dict(y=np.arange(40) % 17), NotImplementedError, "17 classes"),
    "255 features": (dict(X=np.random.default_rng(0).normal(size=(40, 255))), NotImplementedError, "255 features"),
    "depth 0": (dict(depth=0), ValueError, "depth must be"),
    "depth 9": (dict(depth=9), NotImplementedError, "tree depth 9"),
    "border_count 0": (dict(border_count=0), ValueError, "border_count must be"),
    "border_count 256": (dict(border_count=256), NotImplementedError, "border_count 256"),
    "n_trees 0": (dict(n_trees=0), ValueError, "n_trees must be"),
    "lambda 0": (dict(l2_leaf_reg=0.0), ValueError, "l2_leaf_reg must be positive"),
    "lambda nan": (dict(l2_leaf_reg=float("nan")), ValueError, "l2_leaf_reg must be positive"),
    "lr inf": (dict(learning_rate=float("inf")), ValueError, "learning_rate must be finite"),
    "thresholds": (dict(thresholds=np.zeros(7)), ValueError, "one value per class"),
    "status shape": (dict(status=np.zeros(3, np.int32)), ValueError, "status must hold"),
    "label_mapper": (dict(label_mapper={0: 5, 1: 6, 2: 7}), ValueError, "label_mapper must map"),
    "no borders": (dict(X=np.ones((40, 12))), ValueError, "no feature has a border"),
    "no members": (dict(status=np.ones(40, np.int32), y=np.arange(40) % 3), ValueError, "at least two classes"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_fit_refuses_before_any_device_work(name, monkeypatch):
    """with the library's loader disabled, a refusal that needed the device would fail otherwise"""
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the device was reached")))
    monkeypatch.setattr(_lib, "default_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the device was reached")))
    over, exc, text = REFUSALS[name]
    kw = dict(X=np.random.default_rng(0).normal(size=(40, 12)), y=np.arange(40) % 3, n_trees=2, depth=2)
    kw.update(over)
    with pytest.raises(exc, match=text):
        Fpt_Boost.fit(**kw)
