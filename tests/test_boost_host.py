"""Fpt_Boost on the host side: the JSON loader against a literal fixture, the two conventions it fixes (bit order of the
leaf index, layout of leaf_values), every refusal, dispatch and the reference's error strings.  No GPU: the loaded arrays
are evaluated by a few lines of Python that read them exactly as include/wdx.h lays the C ABI out."""
import json
import os
import re
import sys

import numpy as np
import pytest

from helpers import boost_ref
from warpdemux_amd import _lib, models

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = os.path.join(GOLDEN, "boost_tiny.json")
LM2 = {0: 7, 1: 3}

# rows of the tiny model and their raw scores, worked out by hand from the fixture's text:
#   tree 0 (depth 0) adds [0.5, -0.25]; tree 1 tests x1 > 0.5 (NaN: AsTrue); tree 2 tests x0 > 0 for bit 0 and x2 > -1 for
#   bit 1 (NaN: AsFalse); raw = 2 * sum + [0.5, -0.5]
TINY_X = np.array([[1.0, 1.0, 0.0],        # [0.5,-0.25] + [3,4] + leaf 3 [1000,2000] = [1003.5, 2003.75]
                   [1.0, 0.0, -2.0],       # [0.5,-0.25] + [1,2] + leaf 1 [10,20]     = [11.5, 21.75]
                   [-1.0, 0.5, 0.0],       # x1 == border is false: [1,2]; leaf 2 [100,200] -> [101.5, 201.75]
                   [0.0, np.nan, np.nan]])  # x1 NaN AsTrue [3,4]; x0 == 0 false, x2 NaN AsFalse: leaf 0 -> [3.625, 4.0]
TINY_RAW = np.array([[2007.5, 4007.0], [23.5, 43.0], [203.5, 403.0], [7.75, 7.5]])


def abi_raw(fb, X):
    """Raw scores from the arrays that cross the C ABI (wdx_boost_model), read the way include/wdx.h says."""
    x32 = np.asarray(X, dtype=np.float64).astype(np.float32)
    out = np.zeros((len(x32), fb.dim))
    for r, x in enumerate(x32):
        acc = np.zeros(fb.dim)
        s0 = l0 = 0
        for d in fb._depth:
            leaf = 0
            for i in range(d):
                v = x[fb._split_feature[s0 + i]]
                bit = bool(v > fb._split_border[s0 + i]) or (bool(np.isnan(v)) and bool(fb._split_nan_true[s0 + i]))
                leaf |= int(bit) << i
            acc = acc + fb._leaf_values[l0 + leaf * fb.dim: l0 + (leaf + 1) * fb.dim]
            s0 += d
            l0 += (1 << d) * fb.dim
        out[r] = fb.scale * acc + fb._bias
    return out


def tiny_model():
    return boost_ref.BoostModel(
        [([], [], [[0.5, -0.25]]), ([1], [0.5], [[1, 2], [3, 4]]),
         ([0, 2], [0.0, -1.0], [[0.125, 0.25], [10, 20], [100, 200], [1000, 2000]])],
        n_features=3, dim=2, scale=2.0, bias=[0.5, -0.5], nan_treatment=["AsIs", "AsTrue", "AsFalse"])


def test_loader_against_the_literal_fixture():
    fb = models.Fpt_Boost.from_json(TINY, LM2, thresholds=np.array([0.1, 0.2]))
    assert (fb.n_features, fb.dim, fb.k, fb.scale) == (3, 2, 2, 2.0)
    assert fb._depth.tolist() == [0, 1, 2] and fb._depth.dtype == np.int32
    assert fb._split_feature.tolist() == [1, 0, 2] and fb._split_feature.dtype == np.int32
    assert fb._split_border.tolist() == [0.5, 0.0, -1.0] and fb._split_border.dtype == np.float32
    assert fb._split_nan_true.tolist() == [1, 0, 0] and fb._split_nan_true.dtype == np.uint8
    assert fb._leaf_values.tolist() == [0.5, -0.25, 1, 2, 3, 4, 0.125, 0.25, 10, 20, 100, 200, 1000, 2000]
    assert fb._bias.tolist() == [0.5, -0.5] and fb._label_arr.tolist() == [7, 3]
    assert np.array_equal(abi_raw(fb, TINY_X), TINY_RAW)
    m = fb.to_c()
    assert (m.n_trees, m.n_features, m.dim, m.n_classes, m.scale) == (3, 3, 2, 2, 2.0)
    # the parsed dict loads like the path
    with open(TINY) as fh:
        fb2 = models.Fpt_Boost.from_json(json.load(fh), LM2)
    assert np.array_equal(fb2._leaf_values, fb._leaf_values) and fb2.thresholds is None


def test_restatement_and_writer_agree_with_the_fixture():
    m = tiny_model()
    assert np.array_equal(boost_ref.raw_scores(m, TINY_X), TINY_RAW)
    with open(TINY) as fh:
        lit = json.load(fh)
    js = boost_ref.to_json(m)
    assert js["scale_and_bias"] == lit["scale_and_bias"]
    for a, b in zip(js["oblivious_trees"], lit["oblivious_trees"]):
        assert a["leaf_values"] == b["leaf_values"]
        assert [(s["float_feature_index"], s["border"], s["split_type"]) for s in a["splits"]] == \
               [(s["float_feature_index"], s["border"], s["split_type"]) for s in b["splits"]]
    assert [f["nan_value_treatment"] for f in js["features_info"]["float_features"]] == ["AsIs", "AsTrue", "AsFalse"]
    p = boost_ref.predict_proba(m, TINY_X)
    assert np.allclose(p.sum(axis=1), 1) and p[3, 0] > p[3, 1] and p[0, 1] == 1.0


def test_convention_bit_order():
    """splits[i] sets bit i: a model whose two splits, swapped, give another answer -- loader and restatement agree on
    both, and the two differ."""
    m = boost_ref.BoostModel([([0, 1], [0.0, 0.0], [[1.0], [2.0], [4.0], [8.0]])], 2, 1, 1.0, [0.0])
    sw = boost_ref.BoostModel([([1, 0], [0.0, 0.0], [[1.0], [2.0], [4.0], [8.0]])], 2, 1, 1.0, [0.0])
    X = np.array([[1.0, -1.0], [-1.0, 1.0]])       # only x0 > 0 -> bit 0 -> leaf 1; only x1 > 0 -> bit 1 -> leaf 2
    assert boost_ref.raw_scores(m, X).ravel().tolist() == [2.0, 4.0]
    assert boost_ref.raw_scores(sw, X).ravel().tolist() == [4.0, 2.0]
    for mm in (m, sw):
        fb = models.Fpt_Boost.from_json(boost_ref.to_json(mm), LM2)
        assert np.array_equal(abi_raw(fb, X), boost_ref.raw_scores(mm, X))


def test_convention_leaf_layout():
    """leaf_values[leaf * dim + c]: a model for which the transposed reading (class-major) gives another answer."""
    leaves = np.array([[1.0, 2.0, 3.0], [10.0, 20.0, 30.0]])           # (2 leaves, dim 3)
    m = boost_ref.BoostModel([([0], [0.0], leaves)], 1, 3, 1.0, [0.0, 0.0, 0.0])
    X = np.array([[-1.0], [1.0]])
    js = boost_ref.to_json(m)
    assert js["oblivious_trees"][0]["leaf_values"] == [1.0, 2.0, 3.0, 10.0, 20.0, 30.0]
    fb = models.Fpt_Boost.from_json(js, {0: 0, 1: 1, 2: 2})
    assert abi_raw(fb, X).tolist() == [[1.0, 2.0, 3.0], [10.0, 20.0, 30.0]] == boost_ref.raw_scores(m, X).tolist()
    transposed = boost_ref.BoostModel([([0], [0.0], leaves.T.reshape(2, 3))], 1, 3, 1.0, [0.0, 0.0, 0.0])
    assert boost_ref.raw_scores(transposed, X).tolist() == [[1.0, 10.0, 2.0], [20.0, 3.0, 30.0]]


def test_scalar_bias_and_logloss_class_count():
    m = boost_ref.random_model(3, 2, 1, 4, seed=1)
    js = boost_ref.to_json(m)
    js["scale_and_bias"] = [m.scale, float(m.bias[0])]              # the older scalar form
    del js["model_info"]
    fb = models.Fpt_Boost.from_json(js, LM2)
    assert (fb.dim, fb.k) == (1, 2) and fb._bias.tolist() == [float(m.bias[0])]
    X = boost_ref.random_inputs(m, 50, seed=2)
    assert np.array_equal(abi_raw(fb, X), boost_ref.raw_scores(m, X))


def _js(**kw):
    return boost_ref.to_json(boost_ref.random_model(**{**dict(n_trees=2, depth_spec=2, dim=3, n_features=4, seed=0), **kw}))


def test_refusals():
    lm = {i: i for i in range(17)}
    js = _js()
    js["trees"] = js.pop("oblivious_trees")
    with pytest.raises(NotImplementedError, match="non-symmetric"):
        models.Fpt_Boost.from_json(js, lm)
    for key, word in (("categorical_features", "categorical"), ("text_features", "text"), ("embedding_features", "embedding"),
                      ("ctrs", "categorical")):
        js = _js()
        js["features_info"][key] = [{"feature_index": 0}]
        with pytest.raises(NotImplementedError, match=word):
            models.Fpt_Boost.from_json(js, lm)
    js = _js()
    js["oblivious_trees"][1]["splits"][0]["split_type"] = "OnlineCtr"
    with pytest.raises(NotImplementedError, match="OnlineCtr"):
        models.Fpt_Boost.from_json(js, lm)
    with pytest.raises(NotImplementedError, match="17 classes"):
        models.Fpt_Boost.from_json(_js(dim=17, depth_spec=1), lm)
    with pytest.raises(NotImplementedError, match="depth 17"):
        models.Fpt_Boost.from_json(_js(n_trees=1, depth_spec=17, dim=1), lm)
    with pytest.raises(NotImplementedError, match="255 features"):
        models.Fpt_Boost.from_json(_js(n_features=255), lm)
    # the limits themselves load
    assert models.Fpt_Boost.from_json(_js(dim=16, depth_spec=1), lm).k == 16
    assert models.Fpt_Boost.from_json(_js(n_trees=1, depth_spec=16, dim=1), lm)._depth.tolist() == [16]
    assert models.Fpt_Boost.from_json(_js(n_features=254), lm).n_features == 254
    # malformed models are ValueErrors
    js = _js()
    js["oblivious_trees"][1]["leaf_values"] = js["oblivious_trees"][1]["leaf_values"][:-1]
    with pytest.raises(ValueError):
        models.Fpt_Boost.from_json(js, lm)
    js = _js()
    js["oblivious_trees"][0]["splits"][0]["float_feature_index"] = 9
    with pytest.raises(ValueError):
        models.Fpt_Boost.from_json(js, lm)
    js = _js()
    js["features_info"]["float_features"][0]["nan_value_treatment"] = "AsSomethingElse"
    with pytest.raises(NotImplementedError):
        models.Fpt_Boost.from_json(js, lm)


def test_from_reference_dispatch_on_the_stand_in():
    m = boost_ref.random_model(5, [0, 1, 3], 4, 25, seed=3, nan_treatment=["AsTrue"] * 25)
    thr = np.array([0.1, 0.2, 0.3, 0.4])
    ref = boost_ref.Fpt_Boost(m, {0: 4, 1: 9, 2: 2, 3: 11}, thr, n_classes=4)
    assert "catboost" not in sys.modules
    fb = models.from_reference(ref)
    assert "catboost" not in sys.modules
    assert isinstance(fb, models.Fpt_Boost) and fb.num_bcs == 4 and fb._label_arr.tolist() == [4, 9, 2, 11]
    assert np.array_equal(fb.thresholds, thr) and fb._depth.tolist() == [0, 1, 3, 0, 1] and fb._split_nan_true.all()
    X = boost_ref.random_inputs(m, 40, seed=4)
    X[3, 5] = np.nan
    assert np.array_equal(abi_raw(fb, X), boost_ref.raw_scores(m, X))
    assert boost_ref.Fpt_Boost(m, {i: i for i in range(5)}, None, None, noise_class=True).noise_class

    class DTW_Other:
        pass

    with pytest.raises(NotImplementedError, match="DTW_SVM, DTW_MLP and Fpt_Boost"):
        models.from_reference(DTW_Other())


def test_error_strings_of_the_reference():
    m = boost_ref.random_model(2, 2, 3, 5, seed=5)
    lm = {0: 0, 1: 1, 2: 2}
    with pytest.raises(ValueError, match=r"^Model not trained\.$"):
        models.from_reference(boost_ref.Fpt_Boost(None, lm))
    with pytest.raises(ValueError, match=r"^Model not trained\.$"):
        models.Fpt_Boost([], 5, 1.0, [0.0, 0.0, 0.0], lm).predict(np.zeros((1, 5)))
    for empty in (None, {}):
        with pytest.raises(ValueError, match=r"^Label mapper not set\.$"):
            models.from_reference(boost_ref.Fpt_Boost(m, empty)).predict(np.zeros((1, 5)))
    with pytest.raises(ValueError, match="features"):
        models.from_reference(boost_ref.Fpt_Boost(m, lm)).predict(np.zeros((2, 6)))
    with pytest.raises(ValueError, match="thresholds"):
        models.from_reference(boost_ref.Fpt_Boost(m, lm, np.zeros(4)))


def test_abi_struct_and_constants():
    import ctypes

    assert ctypes.sizeof(_lib.BoostModelC) == 16 + 5 * 8 + 8 + 3 * 8
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "wdx.h")).read()
    body = hdr[hdr.index("typedef struct wdx_boost_model {"): hdr.index("} wdx_boost_model;")]
    fields = re.findall(r"^\s*(?:const\s+)?\w+\s+\*?(\w+);", body, flags=re.M)
    assert fields == [f[0] for f in _lib.BoostModelC._fields_]
    assert f"#define WDX_BOOST_MAX_FEATURES {_lib.BOOST_MAX_FEATURES}" in hdr
    assert f"#define WDX_BOOST_MAX_DEPTH {_lib.BOOST_MAX_DEPTH}" in hdr
    for name in ("wdx_boost_set_model", "wdx_boost_predict_dev", "wdx_boost_predict", "wdx_demux_boost_dev"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert _lib.K_BOOST == 10 and _lib.OPT_BOOST_CHUNK_ROWS == 18
