"""scikit-learn's DTW_MLP tail restated in NumPy, an "exact" forward pass, and the accuracy contract of DESIGN.md 4.7.

DTW_MLP.predict (models/dtw_mlp.py:74-93): D = distance_matrix_to(...) (float32) -> model.model.predict_proba(D) ->
process_probs (models/utils.py:45-61).  model.model is an MLPClassifier or a Pipeline of StandardScaler steps and one.

- StandardScaler.transform on float32 input: x - mean_ in float64 rounded to float32, then / scale_ likewise.
- MLPClassifier._forward_pass_fast: working dtype result_type(float32, coefs_[0].dtype); each layer a @ W, then += b;
  hidden activation identity / logistic (expit) / tanh / relu; output softmax (x - row max, exp, / row sum) or, with one
  output unit, logistic and predict_proba = [1 - p, p] with 1 - p in the working dtype.
- process_probs: first maximum, margin top1 - top2 in the working dtype, pred -1 where margin < thresholds[pred_idx]
  (compared in float64).

`exact_proba` runs the same model in float64 (float32 models) or np.longdouble (float64 models) after the scaler steps,
which are part of the input definition and reproduced bit for bit.  Tolerance per case: T = 4 max(E_ref, u_w) with
E_ref = max |p_sklearn - p_exact| (the factor and its reason: DESIGN.md 4.7).
"""
from __future__ import annotations

import copy

import numpy as np
from scipy.special import expit

ACTS = ("identity", "logistic", "tanh", "relu")


def split_model(est):
    """(scaler steps [(mean or None, scale or None)], MLPClassifier)"""
    from sklearn.pipeline import Pipeline

    steps = [s for _, s in est.steps] if isinstance(est, Pipeline) else [est]
    scalers = [(s.mean_ if s.with_mean else None, s.scale_ if s.with_std else None) for s in steps[:-1]]
    return scalers, steps[-1]


def scale(scalers, D):
    """StandardScaler.transform steps on float32 D, bit for bit."""
    X = np.array(D, dtype=np.float32)
    for mean, sc in scalers:
        if mean is not None:
            X = (X.astype(np.float64) - mean).astype(np.float32)
        if sc is not None:
            X = (X.astype(np.float64) / sc).astype(np.float32)
    return X


def _act(name, x):
    if name == "identity":
        return x
    if name == "relu":
        return np.maximum(x, 0)
    if name == "tanh":
        return np.tanh(x)
    if x.dtype == np.longdouble:
        return 1 / (1 + np.exp(-x))
    return expit(x)


def _proba(mlp, X, dt):
    a = X.astype(dt) if dt == np.longdouble else X
    nl = len(mlp.coefs_)
    for i, (W, b) in enumerate(zip(mlp.coefs_, mlp.intercepts_)):
        if dt == np.longdouble:
            W, b = W.astype(dt), b.astype(dt)
        a = a @ W
        a += b
        if i < nl - 1:
            a = _act(mlp.activation, a)
    if mlp.out_activation_ == "logistic":
        p = _act("logistic", a).ravel()
        return np.vstack([1 - p, p]).T
    a = a - a.max(axis=1)[:, None]
    a = np.exp(a)
    return a / a.sum(axis=1)[:, None]


def sklearn_proba(est, D):
    """scikit-learn's predict_proba restated (bitwise on the float64 path)."""
    scalers, mlp = split_model(est)
    X = scale(scalers, D)
    dt = np.result_type(np.float32, mlp.coefs_[0].dtype)
    if dt == np.float64:
        X = X.astype(np.float64)
    return _proba(mlp, X, dt)


def exact_proba(est, D):
    """The same model in float64 (float32 models) or np.longdouble (float64 models); scaler steps bit for bit."""
    scalers, mlp = split_model(est)
    X = scale(scalers, D)
    if mlp.coefs_[0].dtype == np.float64:
        assert np.finfo(np.longdouble).nmant >= 63
        return _proba(mlp, X, np.longdouble)
    return _proba(mlp, X.astype(np.float64), np.float64)


def process_probs(y_prob, label_mapper, thresholds=None):
    """models/utils.py:45-61"""
    pred_idx = np.argmax(y_prob, axis=1)
    pred = np.array([label_mapper[i] for i in pred_idx], dtype=np.int64)
    s = np.sort(y_prob, axis=1)[:, ::-1]
    conf = s[:, 0] - s[:, 1]
    if thresholds is not None:
        pred[conf < thresholds[pred_idx]] = -1
    return pred, conf


def unit_roundoff(dtype):
    return float(np.finfo(dtype).eps) / 2


def contract(est, D, thresholds):
    """Per-case figures: sklearn's and the exact outputs, E_ref, T and the close-call mask."""
    p_sk = est.predict_proba(D)
    p_ex = exact_proba(est, D)
    dt = p_sk.dtype
    e_ref = float(np.max(np.abs(p_sk.astype(np.longdouble) - p_ex))) if len(D) else 0.0
    T = 4 * max(e_ref, unit_roundoff(dt))
    s = np.sort(p_ex, axis=1)[:, ::-1]
    conf_ex = s[:, 0] - s[:, 1]
    close = conf_ex < 2 * T
    if thresholds is not None:
        close |= np.abs(conf_ex - thresholds[np.argmax(p_ex, axis=1)]) < 2 * T
    return dict(p_sk=p_sk, p_ex=p_ex, conf_ex=conf_ex, e_ref=e_ref, T=T, close=close)


def check_outputs(c, prob, conf, pred, pred_sk, dtype):
    """The accuracy contract on (prob, conf, pred) from the device; returns (max |p - p_exact|, list of violations)."""
    bad = []
    err = float(np.max(np.abs(prob.astype(np.longdouble) - c["p_ex"]))) if len(prob) else 0.0
    if not err <= c["T"]:   # (a NaN fails too)
        bad.append(f"max |p - p_exact| = {err:.3g} > T = {c['T']:.3g}")
    cerr = float(np.max(np.abs(conf.astype(np.longdouble) - c["conf_ex"]))) if len(conf) else 0.0
    if not cerr <= 2 * c["T"]:
        bad.append(f"max |conf - conf_exact| = {cerr:.3g} > 2T")
    if dtype == np.float32:
        if not (np.array_equal(prob.astype(np.float32).astype(np.float64), prob)
                and np.array_equal(conf.astype(np.float32).astype(np.float64), conf)):
            bad.append("float32 model returned values that are not float32")
    wrong = (pred != pred_sk) & ~c["close"]
    if wrong.any():
        bad.append(f"{int(wrong.sum())} preds differ outside close calls")
    return err, bad


# ---- model fixtures --------------------------------------------------------------------------------------------------

class DTW_MLP:
    """Stand-in carrying the upstream attributes (models/dtw_base.py:14-25); the class name is what dispatch reads."""

    def __init__(self, model, _X, label_mapper, thresholds=None, window=15, penalty=0.1, block_size=None, n_classes=None,
                 noise_class=False):
        self.model, self._X, self.label_mapper, self.thresholds = model, _X, label_mapper, thresholds
        self.window, self.penalty, self.block_size = window, penalty, block_size
        self.n_classes, self.noise_class = n_classes, noise_class


def random_mlp(n_in, hidden, k, dtype, activation, seed):
    """MLPClassifier fitted for one iteration (for its fitted attributes), then coefs_ ~ N(0, 2 / (fan_in + fan_out)) and
    intercepts_ ~ N(0, 0.1) in `dtype`."""
    import warnings

    from sklearn.neural_network import MLPClassifier

    rng = np.random.default_rng(seed)
    Xf = rng.normal(size=(max(2 * k, 8), n_in)).astype(dtype)
    yf = np.arange(len(Xf)) % k
    m = MLPClassifier(hidden_layer_sizes=hidden, activation=activation, max_iter=1, random_state=seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(Xf, yf)
    m.coefs_ = [rng.normal(0, np.sqrt(2 / (W.shape[0] + W.shape[1])), W.shape).astype(dtype) for W in m.coefs_]
    m.intercepts_ = [rng.normal(0, np.sqrt(0.1), b.shape).astype(dtype) for b in m.intercepts_]
    return m


def trained_mlp(D, y, hidden, dtype, seed):
    """A small genuinely trained model on (D, y)."""
    import warnings

    from sklearn.neural_network import MLPClassifier

    m = MLPClassifier(hidden_layer_sizes=hidden, max_iter=60, random_state=seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(D.astype(dtype), y)
    return m


def with_scaler(m, D, kind):
    """kind: None | "meanstd" | "std": a Pipeline of one StandardScaler fitted on D and the MLP."""
    if kind is None:
        return m
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler

    s = StandardScaler(with_mean=(kind == "meanstd")).fit(D)
    return Pipeline([("scaler", s), ("mlp", m)])


def clustered_distances(n, nY, k, seed, sigma=3.0):
    """Distances around per-class centres U(2, 8) with noise of scale sigma, float32, and the class of each row."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(2, 8, size=(k, nY))
    y = rng.integers(0, k, size=n)
    D = np.abs(centres[y] + rng.normal(0, sigma, size=(n, nY)))
    return D.astype(np.float32), y


def perturb_first_layer(est, D, T):
    """A copy of `est` with one first-layer weight moved until the exact outputs move by >= 10 T on some read."""
    from sklearn.pipeline import Pipeline

    base = exact_proba(est, D)
    delta = 10 * T
    for _ in range(200):
        e2 = copy.deepcopy(est)
        mlp = e2.steps[-1][1] if isinstance(e2, Pipeline) else e2
        W = mlp.coefs_[0]
        W[0, 0] = W.dtype.type(W[0, 0] + delta)
        moved = float(np.max(np.abs(exact_proba(e2, D) - base)))
        if moved >= 10 * T:
            return e2, moved
        delta *= 2
    raise AssertionError("no perturbation moved the outputs")
