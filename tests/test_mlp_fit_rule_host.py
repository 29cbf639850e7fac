"""The training rule of the device MLP trainer and the host code around it, without a GPU.

1. tests/helpers/mlp_fit_rule.py (the NumPy restatement of include/wdx.h's wdx_mlp_fit_device rule) in float64 against
   scikit-learn's ``MLPClassifier(solver="adam")`` on float64 input with the same integer seed: weights and loss curve within
   1e-12 after 6 epochs, on three shapes, one unshuffled fit and one whose batch_size exceeds m (clipped to m).  The observed
   differences are printed.
2. `_mlp_fit.schedule` (the package's own draws) against the restatement's, bit for bit.
3. The stop rule on a hand-made loss curve, and ``tol=1e9, n_iter_no_change=2``: scikit-learn's ``n_iter_`` (four epochs: the
   first epoch is compared with an infinite best and does not count).
4. Every refusal `DTW_MLP.fit` makes before any device work."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import mlp_fit_rule as rule  # noqa: E402
from warpdemux_amd import _lib, _mlp_fit  # noqa: E402
from warpdemux_amd.models import DTW_MLP  # noqa: E402

# name: (rows, features, hidden, activation, classes, batch_size, shuffle)
CASES = {
    "530x37-relu-4": (530, 37, (24,), "relu", 4, 200, True),
    "530x37-tanh-2x2": (530, 37, (24, 10), "tanh", 2, 200, True),
    "203x19-relu-5": (203, 19, (17,), "relu", 5, 64, True),
    "203x19-unshuffled": (203, 19, (17,), "logistic", 5, 64, False),
    "70x5-batch-beyond-m": (70, 5, (3,), "relu", 3, 500, True),
}
EPOCHS, SEED = 6, 7


def problem(m, F, k, seed=0, dtype=np.float64):
    """(X, y_idx): k noisy class templates, already of unit scale"""
    rng = np.random.default_rng(100 + seed + m)
    T = rng.normal(size=(k, F))
    y = rng.integers(0, k, m)
    y[:k] = np.arange(k)
    return (T[y] + 0.8 * rng.normal(size=(m, F))).astype(dtype), y.astype(np.int64)


def sklearn_fit(X, y, hidden, activation, batch, shuffle, epochs=EPOCHS, seed=SEED, **kw):
    from sklearn.neural_network import MLPClassifier

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return MLPClassifier(hidden_layer_sizes=hidden, activation=activation, batch_size=batch, shuffle=shuffle, max_iter=epochs,
                             random_state=seed, **kw).fit(X, y)


@functools.lru_cache(maxsize=None)
def _case(name):
    m, F, hidden, act, k, batch, shuffle = CASES[name]
    X, y = problem(m, F, k)
    sk = sklearn_fit(X, y, hidden, act, batch, shuffle)
    sizes = [F] + list(hidden) + [1 if k == 2 else k]
    W0, B0, order = rule.init_and_order(sizes, act, SEED, m, EPOCHS, shuffle)
    W, B, curve, stopped = rule.fit(X, y, k, W0, B0, order, activation=act, batch_size=batch, max_epochs=EPOCHS)
    return sk, W, B, curve, stopped


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_scikit_learn_in_float64(name):
    sk, W, B, curve, stopped = _case(name)
    dw = max(np.abs(a - b).max() for a, b in zip(W + B, sk.coefs_ + sk.intercepts_))
    dl = np.abs(curve - np.asarray(sk.loss_curve_)).max()
    print(f"{name}: max |weight difference| {dw:.3g}, max |loss difference| {dl:.3g}")
    assert len(curve) == sk.n_iter_ == EPOCHS and not stopped
    assert dw <= 1e-12 and dl <= 1e-12


@pytest.mark.parametrize("name", sorted(CASES))
def test_package_schedule_equals_the_restatement(name):
    m, F, hidden, act, k, batch, shuffle = CASES[name]
    sizes = [F] + list(hidden) + [1 if k == 2 else k]
    assert _mlp_fit.layer_sizes(F, hidden, k) == sizes
    W0, B0, order = rule.init_and_order(sizes, act, SEED, m, EPOCHS, shuffle, dtype=np.float32)
    W1, B1, order1 = _mlp_fit.schedule(sizes, act, SEED, m, EPOCHS, shuffle)
    for a, b in zip(W0 + B0, W1 + B1):
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    if shuffle:
        assert order1.dtype == np.int32 and np.array_equal(order, order1)
        assert all(np.array_equal(np.sort(r), np.arange(m)) for r in order1)
    else:
        assert order is None and order1 is None


def test_stop_rule_on_a_hand_made_curve():
    # best 1.0 -> 0.5; then three epochs within tol of the best: counts 1, 2, 3 > 2 at index 4
    curve = [1.0, 0.5, 0.45, 0.46, 0.47, 0.1]
    for f in (rule.stop_epoch, _mlp_fit.stop_epoch):
        assert f(curve, 0.1, 2) == (4, True)
        assert f(curve, 0.1, 3) == (5, False)
        assert f(curve, 0.01, 0) == (3, True)       # 0.46 > 0.45 - 0.01
        assert f([3.0, 2.0, 1.0], 0.5, 0) == (2, False)


def test_huge_tol_stops_where_scikit_learn_does():
    """tol=1e9, n_iter_no_change=2: every epoch but the first counts as no improvement (the first is compared with an infinite best:
    ``loss > inf - tol`` is false), so scikit-learn 1.7 stops with ``n_iter_`` = 4; the rule must stop at scikit-learn's count"""
    m, F, hidden, act, k, batch, shuffle = CASES["203x19-relu-5"]
    X, y = problem(m, F, k)
    sk = sklearn_fit(X, y, hidden, act, batch, shuffle, epochs=50, tol=1e9, n_iter_no_change=2)
    sizes = [F] + list(hidden) + [k]
    W0, B0, order = rule.init_and_order(sizes, act, SEED, m, 50, shuffle)
    W, B, curve, stopped = rule.fit(X, y, k, W0, B0, order, activation=act, batch_size=batch, max_epochs=50, tol=1e9, n_iter_no_change=2)
    assert sk.n_iter_ == len(curve) == 4 and stopped
    assert rule.stop_epoch(sk.loss_curve_, 1e9, 2) == _mlp_fit.stop_epoch(sk.loss_curve_, 1e9, 2) == (sk.n_iter_ - 1, True)
    assert max(np.abs(a - b).max() for a, b in zip(W + B, sk.coefs_ + sk.intercepts_)) <= 1e-12


def test_float32_restatement_stays_near_the_float64_one():
    """the float32 run, every product accumulated strictly in k order, against float64: rounding only (the issue's 2e-7 after 10
    epochs was measured on these shapes; 1e-5 here is a sanity bound, not the device contract)"""
    m, F, hidden, act, k, batch, shuffle = CASES["203x19-relu-5"]
    X, y = problem(m, F, k)
    sizes = [F] + list(hidden) + [k]
    W0, B0, order = rule.init_and_order(sizes, act, SEED, m, EPOCHS, shuffle)
    W64, B64, c64, _ = rule.fit(X.astype(np.float32).astype(np.float64), y, k, W0, B0, order, activation=act, batch_size=batch, max_epochs=EPOCHS)
    W32, B32, c32, _ = rule.fit(X.astype(np.float32), y, k, W0, B0, order, activation=act, batch_size=batch, max_epochs=EPOCHS, ordered=True)
    assert all(w.dtype == np.float32 for w in W32 + B32)
    d = max(np.abs(a - b).max() for a, b in zip(W64 + B64, W32 + B32))
    print(f"float32 ordered against float64: {d:.3g}")
    assert d <= 1e-5 and np.abs(c32 - c64).max() <= 1e-5


def test_constants_agree_across_the_layers():
    import re

    hdr = open(os.path.join(ROOT, "include", "wdx.h")).read()
    assert int(re.search(r"#define\s+WDX_MLP_FIT_MAX_BATCH\s+(\d+)", hdr).group(1)) == _lib.MLP_FIT_MAX_BATCH >= 256
    assert int(re.search(r"#define\s+WDX_K_MLP_FIT\s+(\d+)", hdr).group(1)) == _lib.K_MLP_FIT == 16
    for i, name in enumerate(_lib.MLP_FIT_STATES):
        assert int(re.search(r"#define\s+WDX_MLP_FIT_%s\s+(\d+)" % name.upper(), hdr).group(1)) == i
    assert "wdx_mlp_fit_device" in _lib.EXPORTS and "wdx_mlp_fit" in _lib.EXPORTS
    import ctypes as C

    assert C.sizeof(_lib.MlpFitParamsC) == 4 * 12 + 8 * 6


REFUSALS = {
    "X not 2-d": (dict(X=np.zeros(5)), ValueError, "X must be"),
    "y shape": (dict(y=np.zeros(3, np.int64)), ValueError, "one label per row"),
    "y dtype": (dict(y=np.zeros(40)), ValueError, "integer dtype"),
    "one class": (dict(y=np.zeros(40, np.int64)), ValueError, "at least two classes"),
    "17 classes": (dict(y=np.arange(40) % 17), ValueError, "at most 16"),
    "refs shape": (dict(refs=np.zeros((3, 5))), ValueError, "refs must be"),
    "distances shape": (dict(distances=np.zeros((40, 3), np.float32)), ValueError, "distances must be"),
    "solver": (dict(solver="lbfgs"), ValueError, "solver must be"),
    "activation": (dict(activation="gelu"), ValueError, "unknown activation"),
    "tol": (dict(tol=0.0), ValueError, "tol must be positive"),
    "learning rate": (dict(learning_rate_init=-1e-3), ValueError, "learning_rate_init must be positive"),
    "batch_size": (dict(batch_size=0), ValueError, "batch_size must be"),
    "batch beyond the cap": (dict(batch_size=_lib.MLP_FIT_MAX_BATCH + 1), NotImplementedError, "WDX_MLP_FIT_MAX_BATCH"),
    "hidden width": (dict(hidden_layer_sizes=(_lib.MLP_MAX_WIDTH + 1,)), NotImplementedError, "at most 512"),
    "hidden layers": (dict(hidden_layer_sizes=(8,) * _lib.MLP_MAX_LAYERS), NotImplementedError, "hidden layers"),
    "hidden empty": (dict(hidden_layer_sizes=()), ValueError, "hidden_layer_sizes"),
    "seed": (dict(random_state=None), ValueError, "non-negative integer random_state"),
    "negative seed": (dict(random_state=-1), ValueError, "non-negative integer random_state"),
    "thresholds": (dict(thresholds=np.zeros(7)), ValueError, "one value per class"),
    "max_iter": (dict(max_iter=0), ValueError, "max_iter must be"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_fit_refuses_before_any_device_work(name, monkeypatch):
    """with `distances` given and the library's loader disabled, a refusal that needed the device would fail otherwise"""
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the device was reached")))
    monkeypatch.setattr(_lib, "default_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the device was reached")))
    over, exc, text = REFUSALS[name]
    kw = dict(X=np.random.default_rng(0).normal(size=(40, 12)), y=np.arange(40) % 3, window=3, penalty=0.1,
              distances=np.ones((40, 40), np.float32))
    kw.update(over)
    with pytest.raises(exc, match=text):
        DTW_MLP.fit(**kw)
