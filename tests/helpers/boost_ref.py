"""The Fpt_Boost tail restated in NumPy: the defining document of wdx_boost.hip.

Fpt_Boost.predict (models/fpt_boost.py:14-52) is ``model.predict_proba(X)`` of a CatBoost classifier on the raw fingerprint,
then process_probs (models/utils.py:45-61).  CatBoost is not available where this project is built and tested, so nothing
here is compared with it: this file is written from CatBoost's published JSON model format and its published recipe for
applying a JSON model, and the device kernel is held to THIS file.  Parity with CatBoost itself is unpinned (the
opportunistic test in test_gpu_boost.py pins it the day the library is importable).

The model: oblivious (symmetric) trees over float features.
- features are float32: the float64 fingerprint is rounded once;
- level i of a tree tests one (feature, border) pair: ``x > border`` in float32 (equality is false); a NaN feature gives
  false under the feature's nan_value_treatment "AsIs" / "AsFalse" and true under "AsTrue";
- CONVENTION 1: ``splits[i]`` sets bit i of the leaf index;
- CONVENTION 2: ``leaf_values`` is leaf-major with the class dimension fastest: ``leaf_values[leaf * dim + c]``;
- raw_c = scale * (sum over trees of leaf_c, tree 0 first, one float64 add per tree) + bias_c, a float64 multiply and then a
  float64 add;
- dim == k (MultiClass): softmax with the row maximum subtracted, exp and the class-order sum in float64;
  dim == 1, k == 2 (Logloss): p1 = 1 / (1 + exp(-raw)), p = [1 - p1, p1].

Accuracy contract of the probabilities (the raw scores are bit for bit): E_ref = max |p_f64 - p_longdouble| of this
restatement on the case, T = 4 max(E_ref, 2**-53) (the factor DESIGN.md 4.7 measured for an exp-and-normalise epilogue).
"""
from __future__ import annotations

import copy
import json

import numpy as np

from .mlp_ref import process_probs  # noqa: F401  (models/utils.py:45-61, shared with the MLP tail)

NAN_TREATMENTS = ("AsIs", "AsFalse", "AsTrue")


class BoostModel:
    """trees: list of (features int[depth], borders float32[depth], leaves float64 (2**depth, dim)); nan_treatment: one of
    NAN_TREATMENTS per feature."""

    def __init__(self, trees, n_features, dim, scale, bias, nan_treatment=None):
        self.trees = [(np.asarray(f, dtype=np.int64), np.asarray(b, dtype=np.float32), np.asarray(lv, dtype=np.float64))
                      for f, b, lv in trees]
        self.n_features, self.dim = int(n_features), int(dim)
        self.k = 2 if dim == 1 else int(dim)
        self.scale = float(scale)
        self.bias = np.asarray(bias, dtype=np.float64).reshape(dim)
        self.nan_treatment = list(nan_treatment) if nan_treatment is not None else ["AsIs"] * self.n_features
        for f, b, lv in self.trees:
            assert lv.shape == (1 << len(f), dim) and len(f) == len(b)


def leaf_indices(m: BoostModel, X):
    """(n_trees, n) leaf index of every row in every tree."""
    x32 = np.asarray(X, dtype=np.float64).astype(np.float32)
    out = np.zeros((len(m.trees), len(x32)), dtype=np.int64)
    for t, (feat, border, _) in enumerate(m.trees):
        for i, (f, b) in enumerate(zip(feat, border)):
            x = x32[:, f]
            with np.errstate(invalid="ignore"):
                bit = x > b                                   # float32 compare; NaN and equality are false
            if m.nan_treatment[f] == "AsTrue":
                bit = bit | np.isnan(x)
            out[t] |= bit.astype(np.int64) << i               # CONVENTION 1
    return out


def raw_scores(m: BoostModel, X):
    """(n, dim) float64, the sequential loop the kernel reproduces bit for bit."""
    idx = leaf_indices(m, X)
    acc = np.zeros((idx.shape[1], m.dim), dtype=np.float64)
    for t, (_, _, leaves) in enumerate(m.trees):
        acc = acc + leaves[idx[t]]                            # one float64 add per tree, tree 0 first
    return m.scale * acc + m.bias                             # multiply, then add: two roundings


def proba_from_raw(raw, dtype=np.float64):
    """(n, k) probabilities of float64 raw scores, the epilogue evaluated in `dtype` (float64 or np.longdouble)."""
    z = np.asarray(raw, dtype=np.float64).astype(dtype)
    one = dtype(1)
    if z.shape[1] == 1:
        p1 = one / (one + np.exp(-z[:, 0]))
        return np.stack([one - p1, p1], axis=1)
    e = np.exp(z - z.max(axis=1)[:, None])
    s = np.zeros(len(z), dtype=dtype)
    for c in range(z.shape[1]):                               # class order, as one lane adds them
        s = s + e[:, c]
    return e / s[:, None]


def predict_proba(m: BoostModel, X, dtype=np.float64):
    return proba_from_raw(raw_scores(m, X), dtype)


def contract(m: BoostModel, X, thresholds=None):
    """Per-case figures: raw, the float64 and the exact (longdouble) probabilities, E_ref, T and the close-call mask."""
    assert np.finfo(np.longdouble).nmant >= 63
    raw = raw_scores(m, X)
    p64 = proba_from_raw(raw, np.float64)
    p_ex = proba_from_raw(raw, np.longdouble)
    e_ref = float(np.max(np.abs(p64.astype(np.longdouble) - p_ex))) if len(raw) else 0.0
    T = 4 * max(e_ref, 2.0 ** -53)
    s = np.sort(p_ex, axis=1)[:, ::-1]
    conf_ex = s[:, 0] - s[:, 1]
    close = conf_ex < 2 * T
    if thresholds is not None:
        close = close | (np.abs(conf_ex - np.asarray(thresholds)[np.argmax(p_ex, axis=1)]) < 2 * T)
    return dict(raw=raw, p64=p64, p_ex=p_ex, conf_ex=conf_ex, e_ref=e_ref, T=T, close=close)


def check_outputs(c, prob, conf, pred, pred_ref):
    """The accuracy contract on the device's (prob, conf, pred); returns (max |p - p_exact|, list of violations)."""
    bad = []
    err = float(np.max(np.abs(prob.astype(np.longdouble) - c["p_ex"]))) if len(prob) else 0.0
    if not err <= c["T"]:   # (a NaN fails too)
        bad.append(f"max |p - p_exact| = {err:.3g} > T = {c['T']:.3g}")
    cerr = float(np.max(np.abs(conf.astype(np.longdouble) - c["conf_ex"]))) if len(conf) else 0.0
    if not cerr <= 2 * c["T"]:
        bad.append(f"max |conf - conf_exact| = {cerr:.3g} > 2T")
    wrong = (pred != pred_ref) & ~c["close"]
    if wrong.any():
        bad.append(f"{int(wrong.sum())} preds differ outside close calls")
    return err, bad


# ---- model fixtures --------------------------------------------------------------------------------------------------

def random_model(n_trees, depth_spec, dim, n_features, seed, nan_treatment=None):
    """depth_spec: one depth for every tree, or a sequence cycled over the trees ("mixed").  Inputs are N(0, 1) per feature
    (random_inputs), and the borders are drawn from that range (float32 of U(-1.5, 1.5)) so that both branches are taken;
    leaves ~ N(0, 4 / n_trees), scale in [0.5, 1.5], bias ~ N(0, 0.25)."""
    rng = np.random.default_rng(seed)
    depths = [depth_spec] * n_trees if np.isscalar(depth_spec) else [depth_spec[t % len(depth_spec)] for t in range(n_trees)]
    trees = []
    for d in depths:
        trees.append((rng.integers(0, n_features, d), rng.uniform(-1.5, 1.5, d).astype(np.float32),
                      rng.normal(0, 2 / np.sqrt(n_trees), (1 << d, dim))))
    return BoostModel(trees, n_features, dim, rng.uniform(0.5, 1.5), rng.normal(0, 0.5, dim), nan_treatment)


def random_inputs(m: BoostModel, n, seed):
    return np.random.default_rng(seed).normal(size=(n, m.n_features))


def to_json(m: BoostModel) -> dict:
    """The model as CatBoost writes it with save_model(format="json") -- the keys the loader reads, plus what surrounds them."""
    borders = [sorted({float(b) for f, bb, _ in m.trees for ff, b in zip(f, bb) if ff == i}) for i in range(m.n_features)]
    return {
        "features_info": {"float_features": [
            {"borders": borders[i], "feature_index": i, "flat_feature_index": i, "has_nans": m.nan_treatment[i] != "AsIs",
             "nan_value_treatment": m.nan_treatment[i]} for i in range(m.n_features)]},
        "model_info": {"class_params": {"class_names": list(range(m.k))},
                       "params": {"loss_function": {"type": "Logloss" if m.dim == 1 else "MultiClass"}}},
        "oblivious_trees": [
            {"leaf_values": [float(v) for v in lv.reshape(-1)],                       # CONVENTION 2: leaf * dim + c
             "leaf_weights": [1] * len(lv),
             "splits": [{"border": float(b), "float_feature_index": int(ff), "split_index": i, "split_type": "FloatFeature"}
                        for i, (ff, b) in enumerate(zip(f, bb))]}
            for f, bb, lv in m.trees],
        "scale_and_bias": [m.scale, [float(v) for v in m.bias]],
    }


def from_json(js: dict) -> BoostModel:
    """The restatement's own reading of a CatBoost JSON model (float features, oblivious trees): the second and last place
    where the two conventions are written down (the first: warpdemux_amd.models.Fpt_Boost.from_json)."""
    ff = js["features_info"]["float_features"]
    col = [int(f.get("flat_feature_index", i)) for i, f in enumerate(ff)]
    n_features = max(col) + 1
    nan = ["AsIs"] * n_features
    for f, c in zip(ff, col):
        nan[c] = f.get("nan_value_treatment", "AsIs")
    scale, bias = js["scale_and_bias"]
    bias = np.atleast_1d(np.asarray(bias, dtype=np.float64))
    d0 = len(js["oblivious_trees"][0]["splits"])
    dim = len(js["oblivious_trees"][0]["leaf_values"]) >> d0
    trees = [([col[s["float_feature_index"]] for s in t["splits"]], [np.float32(s["border"]) for s in t["splits"]],
              np.asarray(t["leaf_values"], dtype=np.float64).reshape(1 << len(t["splits"]), dim))
             for t in js["oblivious_trees"]]
    return BoostModel(trees, n_features, dim, scale, np.resize(bias, dim), nan)


class JsonBackedClassifier:
    """What Fpt_Boost.from_reference asks of ``model.model``: save_model(path, format="json")."""

    def __init__(self, m: BoostModel):
        self._m = m

    def save_model(self, path, format="cbm"):   # noqa: A002  (CatBoost's own keyword)
        if format != "json":
            raise ValueError(f"the stand-in writes JSON only, not {format!r}")
        with open(path, "w") as fh:
            json.dump(to_json(self._m), fh)


class Fpt_Boost:
    """Stand-in carrying the upstream attributes (models/fpt_base.py:11-29); the class name is what dispatch reads."""

    def __init__(self, m, label_mapper, thresholds=None, n_classes=None, noise_class=False):
        self.model = None if m is None else JsonBackedClassifier(m)
        self.label_mapper, self.thresholds = label_mapper, thresholds
        self.n_classes, self.noise_class = n_classes, noise_class


def perturb_leaf(m: BoostModel, X, T):
    """A copy of `m` with one leaf value (tree 0, the leaf of row 0, class 0) moved until the exact outputs move by >= 10 T
    on some read."""
    base = predict_proba(m, X, np.longdouble)
    leaf = int(leaf_indices(m, X)[0, 0])
    delta = 10 * T
    for _ in range(200):
        m2 = copy.deepcopy(m)
        m2.trees[0][2][leaf, 0] += delta
        moved = float(np.max(np.abs(predict_proba(m2, X, np.longdouble) - base)))
        if moved >= 10 * T:
            return m2, moved
        delta *= 2
    raise AssertionError("no perturbation moved the outputs")
