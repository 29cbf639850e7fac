"""The device Fpt_Boost trainer (include/wdx.h: wdx_boost_fit_device, wdx_boost_fit; DemuxEngine.boost_fit; models.Fpt_Boost.fit)
against its NumPy restatement (tests/helpers/boost_fit_rule.py).

Every comparison is ``np.array_equal``: split features, border indices and values, leaf values and scores.  The rule makes that
possible -- quantised gradients, integer histograms, a stated exp, one operation order per float64 expression.

The edge shapes are a covering set over n in {1, 63, 64, 65, R - 1, R, R + 1, 3 R + 5} (R: the rows of one histogram workgroup
pass, `_lib.BOOST_FIT_ROWS`, which tests/test_boost_fit_plan_host.py ties to the plan's), F in {1, 25, 254}, k in {2, 4, 16},
depth in {1, 6, 8} and border_count in {1, 32, 255}: 25 cases, not the full product, in which every listed value of every
parameter occurs (a test asserts that), one tree each.  A single row has no border of its own (the rule and the library refuse
that fit: a test of its own), so the n = 1 cases run on borders the caller supplies, which wdx_boost_fit_device admits: the
histogram, scan and update kernels see the one-row chunk."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import boost_fit_rule as rule  # noqa: E402
from helpers import boost_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LR, LAM = 0.3, 3.0


def _imports():
    global torch, _lib, _boost_fit, models, DemuxEngine
    import torch
    from warpdemux_amd import _boost_fit, _lib, models
    from warpdemux_amd.engine import DemuxEngine


@pytest.fixture(scope="module")
def eng():
    _imports()
    e = DemuxEngine(np.random.default_rng(0).normal(size=(4, 25)), 15, 0.1)
    yield e
    e.close()


def device_fit(eng, X, y, k, n_trees, depth, B, scores=None, border_list=None, lr=LR, lam=LAM, ld_extra=0):
    """(FitTrees, scores as a host array, the borders) through DemuxEngine.boost_fit"""
    n, F = X.shape
    border_list = _boost_fit.borders(X, B) if border_list is None else border_list
    wide = torch.full((n, F + ld_extra), float("nan"), dtype=torch.float64, device=eng.tdev)
    wide[:, :F] = torch.from_numpy(np.ascontiguousarray(X)).to(eng.tdev)
    Xd = wide[:, :F]
    yd = torch.from_numpy(np.asarray(y, dtype=np.int32)).to(eng.tdev)
    Sd = torch.zeros((n, k), dtype=torch.float64, device=eng.tdev) if scores is None else torch.from_numpy(scores.copy()).to(eng.tdev)
    fit = eng.boost_fit(Xd, yd, border_list, Sd, n_trees=n_trees, depth=depth, learning_rate=lr, l2_leaf_reg=lam, border_count=B)
    return fit, Sd.cpu().numpy(), border_list


def assert_same(fit, S, ref, S_ref, border_list):
    for t in range(len(ref.split_feature)):
        assert np.array_equal(fit.split_feature[t], ref.split_feature[t]), (t, fit.split_feature[t], ref.split_feature[t])
        assert np.array_equal(fit.split_border[t], ref.split_border[t]), (t, fit.split_border[t], ref.split_border[t])
        assert np.array_equal(fit.leaf_values[t], ref.leaf_values[t]), t
    assert len(fit.split_feature) == len(ref.split_feature)
    assert all(np.array_equal(a, b) for a, b in zip(border_list, ref.borders))
    assert np.array_equal(S, S_ref)


# ---- stepping tree by tree through the in/out scores ----------------------------------------------------------------------------------

def test_stepping_tree_by_tree(eng):
    X, y = rule.synthetic(300, 8, 3, seed=1)
    S_dev, S_ref = None, None
    for t in range(5):
        fit, S_dev, bl = device_fit(eng, X, y, 3, 1, 3, 16, scores=S_dev)
        ref, S_ref = rule.fit(X, y, 3, 1, 3, LR, LAM, 16, scores=S_ref)
        assert_same(fit, S_dev, ref, S_ref, bl)
    whole, S_whole = rule.fit(X, y, 3, 5, 3, LR, LAM, 16)
    assert np.array_equal(S_whole, S_dev)


# ---- histogram and chunk edges, one tree each ----------------------------------------------------------------------------------------

def _edges():
    from warpdemux_amd import _lib as L

    R = L.BOOST_FIT_ROWS
    return [  # n, F, k, depth, border_count
        (1, 25, 4, 1, 32), (63, 1, 2, 1, 1), (64, 25, 4, 6, 32), (65, 254, 16, 8, 255), (R - 1, 25, 4, 6, 32), (R, 1, 16, 8, 255),
        (R + 1, 25, 2, 1, 255), (3 * R + 5, 25, 4, 6, 32), (3 * R + 5, 254, 2, 1, 1), (63, 25, 16, 6, 1), (64, 1, 4, 8, 32),
        (65, 25, 2, 8, 32), (R, 254, 4, 1, 32), (R + 1, 1, 4, 6, 1), (R - 1, 254, 2, 6, 255), (3 * R + 5, 1, 16, 6, 255),
        (64, 254, 2, 6, 1), (65, 1, 16, 1, 32), (R, 25, 16, 6, 32), (R + 1, 25, 16, 8, 255), (63, 254, 4, 8, 32), (R - 1, 1, 2, 8, 1),
        (3 * R + 5, 25, 2, 8, 1), (64, 25, 16, 1, 255), (1, 1, 2, 8, 255),
    ]


EDGES = _edges()


def test_the_edges_cover_every_value():
    from warpdemux_amd import _lib as L

    R = L.BOOST_FIT_ROWS
    assert R * (1 << L.BOOST_FIT_GRAD_BITS) < 1 << 31
    assert {e[0] for e in EDGES} == {1, 63, 64, 65, R - 1, R, R + 1, 3 * R + 5}
    assert {e[1] for e in EDGES} == {1, 25, 254} and {e[2] for e in EDGES} == {2, 4, 16}
    assert {e[3] for e in EDGES} == {1, 6, 8} and {e[4] for e in EDGES} == {1, 32, 255}
    assert 20 <= len(EDGES) <= 30


@functools.lru_cache(maxsize=None)
def edge_reference(case):
    n, F, k, D, B = case
    X, y = rule.synthetic(n, F, k, seed=n + F + k + D + B)
    bl = None
    if n == 1:   # borders of the caller's: min(B, 3) per feature around the row's value, so that the row falls into bin 0, 1, 2 or 3
        x32 = rule.to_f32(X)[0]
        bl = [(x32[f] + np.arange(min(B, 3), dtype=np.float32) - np.float32((f + 1) % 4) + np.float32(0.5)).astype(np.float32) for f in range(F)]
    ref, S = rule.fit(X, y, k, 1, D, LR, LAM, B, border_list=bl)
    return X, y, ref, S, bl


@pytest.mark.parametrize("case", EDGES, ids=lambda c: "n%d-F%d-k%d-D%d-B%d" % c)
def test_edges(eng, case):
    n, F, k, D, B = case
    X, y, ref, S_ref, bl = edge_reference(case)
    fit, S, bl = device_fit(eng, X, y, k, 1, D, B, border_list=bl)
    assert_same(fit, S, ref, S_ref, bl)
    if n == 1:
        assert np.count_nonzero(fit.leaf_values[0].any(axis=1)) == 1   # the one row's leaf


def test_a_single_row_has_no_border_of_its_own(eng):
    X, y = rule.synthetic(1, 25, 4, seed=9)
    with pytest.raises(rule.Refused):
        rule.fit(X, y, 4, 1, 1, LR, LAM, 32)
    with pytest.raises(ValueError, match="no feature has a border"):
        device_fit(eng, X, y, 4, 1, 1, 32)


# ---- hard inputs ----------------------------------------------------------------------------------------------------------------------

def _hard(name):
    X, y = rule.synthetic(400, 6, 3, seed=21)
    k, D, B, T = 3, 4, 16, 3
    if name == "two identical columns":
        X[:, 4] = X[:, 1]
        X[:, 5] = X[:, 1]
    elif name == "a constant feature":
        X[:, 0] = -2.0
        X[:, 3] = np.nan
    elif name == "a feature with NaNs":
        X[::3, 2] = np.nan
        X[1::5, 0] = np.nan
    elif name == "depth 8 on 65 rows":
        X, y = rule.synthetic(65, 6, 3, seed=22)
        D = 8
    elif name == "all rows of one class":
        y = np.full(400, 1)
    elif name == "coarse features":   # many equal scores: the first maximum decides
        X = np.round(X / 2.0)
        B = 4
    elif name == "a strided X":
        pass
    return X, y, k, T, D, B


HARD = ["two identical columns", "a constant feature", "a feature with NaNs", "depth 8 on 65 rows", "all rows of one class",
        "coarse features", "a strided X"]


@pytest.mark.parametrize("name", HARD)
def test_hard_inputs(eng, name):
    X, y, k, T, D, B = _hard(name)
    ref, S_ref = rule.fit(X, y, k, T, D, LR, LAM, B)
    fit, S, bl = device_fit(eng, X, y, k, T, D, B, ld_extra=5 if name == "a strided X" else 0)
    assert_same(fit, S, ref, S_ref, bl)
    if name == "two identical columns":   # the tie goes to the lower feature
        assert 1 in fit.split_feature and 4 not in fit.split_feature and 5 not in fit.split_feature
    if name == "a constant feature":
        assert len(bl[0]) == 0 and len(bl[3]) == 0 and 0 not in fit.split_feature and 3 not in fit.split_feature
    if name == "depth 8 on 65 rows":     # mostly empty leaves come out 0
        assert (fit.leaf_values[0] == 0).all(axis=1).sum() >= 256 - 65


# ---- a whole fit, the tie to the existing tail, determinism ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def whole():
    X, y = rule.synthetic(2000, 25, 4, seed=3)
    ref, S = rule.fit(X, y, 4, 20, 6, LR, LAM, 32)
    return X, y, ref, S


@pytest.fixture(scope="module")
def whole_model(eng):
    X, y, _, _ = whole()
    return models.Fpt_Boost.fit(X, y, n_trees=20, depth=6, learning_rate=LR, l2_leaf_reg=LAM, border_count=32)


def test_a_whole_fit(eng, whole_model):
    X, y, ref, S_ref = whole()
    m = whole_model
    assert np.array_equal(m.train_scores, S_ref)
    trees = ref.trees()
    assert len(trees) == 20 and np.array_equal(m._depth, np.full(20, 6))
    assert np.array_equal(m._split_feature, np.concatenate([t[0] for t in trees]))
    assert np.array_equal(m._split_border, np.concatenate([t[1] for t in trees]))
    assert np.array_equal(m._leaf_values, np.concatenate([t[2].ravel() for t in trees]))
    assert not m._split_nan_true.any() and m.scale == 1.0 and not m._bias.any() and m.dim == m.k == 4
    assert m.label_mapper == {0: 0, 1: 1, 2: 2, 3: 3} and m.n_dropped_ == 0
    # the device-tensor entry gives the same bits as the host entry
    fit, S, bl = device_fit(eng, X, y, 4, 20, 6, 32)
    assert_same(fit, S, ref, S_ref, bl)


def test_the_tie_to_the_existing_tail(whole_model):
    """the trainer's final scores are what the resident tail computes on the training rows, bit for bit"""
    X, _, _, _ = whole()
    raw = whole_model.predict_raw(X)[0]
    assert np.array_equal(raw, whole_model.train_scores)


def test_two_fits_give_the_same_bits(whole_model):
    X, y, _, _ = whole()
    again = models.Fpt_Boost.fit(X, y, n_trees=20, depth=6, learning_rate=LR, l2_leaf_reg=LAM, border_count=32)
    for name in ("_split_feature", "_split_border", "_leaf_values", "train_scores"):
        a, b = getattr(whole_model, name), getattr(again, name)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name


def test_status_drops_rows_and_labels_are_mapped(eng):
    X, y = rule.synthetic(500, 7, 3, seed=8)
    labels = np.array([11, 5, 42])[y]
    status = (np.arange(500) % 9 == 0).astype(np.int32)
    m = models.Fpt_Boost.fit(X, labels, n_trees=3, depth=3, learning_rate=LR, l2_leaf_reg=LAM, border_count=16, status=status)
    keep = status == 0
    classes = np.array([5, 11, 42])
    ref, S_ref = rule.fit(X[keep], np.searchsorted(classes, labels[keep]), 3, 3, 3, LR, LAM, 16)
    assert m.n_dropped_ == int(status.sum()) and m.label_mapper == {0: 5, 1: 11, 2: 42}
    assert np.array_equal(m.train_scores, S_ref)
    pred, _ = m.predict(X[keep])
    assert np.array_equal(pred, classes[np.argmax(S_ref, axis=1)])


# ---- refusals, the timer ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_and_a_resident_model_usable(eng):
    X, y = rule.synthetic(200, 5, 3, seed=4)
    resident = boost_ref.random_model(7, 3, 3, 5, seed=2)
    dm = models.Fpt_Boost([(f, b, np.zeros(len(f), np.uint8), lv) for f, b, lv in resident.trees], 5, resident.scale, resident.bias,
                          {i: i for i in range(3)})
    eng.set_boost(dm)
    Xd = torch.from_numpy(X).to(eng.tdev)
    before = [t.cpu().numpy() for t in eng.boost_predict(Xd, want_raw=True)]
    bl = _boost_fit.borders(X, 16)
    yd = torch.from_numpy(y.astype(np.int32)).to(eng.tdev)
    Sd = torch.zeros((200, 3), dtype=torch.float64, device=eng.tdev)

    def fit(**kw):
        args = dict(X=Xd, y_idx=yd, borders=bl, scores=Sd, n_trees=1, depth=2, learning_rate=LR, l2_leaf_reg=LAM, border_count=16)
        args.update(kw)
        return eng.boost_fit(args.pop("X"), args.pop("y_idx"), args.pop("borders"), args.pop("scores"), **args)

    eng.kernel_timing(True)
    try:
        eng.kernel_time_reset()
        bad_y = yd.clone()
        bad_y[77] = 3
        neg_y = yd.clone()
        neg_y[0] = -1
        for exc, text, kw in [
            (NotImplementedError, "tree depth 9", dict(depth=9)),
            (ValueError, "depth must be", dict(depth=0)),
            (NotImplementedError, "border_count 256", dict(border_count=256)),
            (ValueError, "n_trees must be", dict(n_trees=0)),
            (ValueError, "l2_leaf_reg", dict(l2_leaf_reg=0.0)),
            (ValueError, "l2_leaf_reg", dict(l2_leaf_reg=-3.0)),
            (ValueError, "learning_rate", dict(learning_rate=float("nan"))),
            (ValueError, "X must be", dict(X=Xd.float())),
            (ValueError, "X must be", dict(X=Xd.t())),
            (ValueError, "y_idx must be", dict(y_idx=yd.long())),
            (ValueError, "scores must be", dict(scores=Sd[:-1])),
            (ValueError, "one array per feature", dict(borders=bl[:-1])),
            (ValueError, "strictly ascending", dict(borders=[b[::-1] for b in bl])),
            (ValueError, "n_borders\\[0\\] = 16 lies outside", dict(border_count=15)),
            (ValueError, "no feature has a border", dict(borders=[np.zeros(0, np.float32)] * 5)),
            (NotImplementedError, "17 classes", dict(scores=torch.zeros((200, 17), dtype=torch.float64, device=eng.tdev))),
            (ValueError, "at least two", dict(scores=torch.zeros((200, 1), dtype=torch.float64, device=eng.tdev))),
        ]:
            with pytest.raises(exc, match=text):
                fit(**kw)
        # the library's own refusals, past the Python checks: the plan's message comes back as the mapped exception
        flat, nb = _boost_fit.pack_borders(bl)
        p = _boost_fit.params_c(5, 3, 1, 2, 16, LR, LAM)
        out = [np.zeros((1, 2), np.int32), np.zeros((1, 2), np.int32), np.zeros((1, 4, 3))]

        def raw(q=p, n=200, ld=5, Xp=Xd.data_ptr(), yp=yd.data_ptr(), Sp=Sd.data_ptr(), o=out, borders_p=None):
            vp = C.c_void_p
            return _lib.check(eng.L.wdx_boost_fit_device(eng.ctx.handle, vp(Xp), n, ld, vp(yp), _lib.ptr(flat) if borders_p is None else borders_p,
                                                         _lib.ptr(nb), C.byref(q), vp(Sp), _lib.ptr(o[0]), _lib.ptr(o[1]), _lib.ptr(o[2]), eng._stream()))

        for field, value, exc, text in [("depth", 9, NotImplementedError, "WDX_BOOST_FIT_MAX_DEPTH"), ("n_classes", 17, NotImplementedError, "17 classes"),
                                        ("n_features", 255, NotImplementedError, "255 features"), ("border_count", 256, NotImplementedError, "WDX_BOOST_FIT_MAX_BORDERS"),
                                        ("n_trees", (1 << 20) + 1, NotImplementedError, "WDX_BOOST_FIT_MAX_TREES"), ("l2_leaf_reg", 0.0, ValueError, "l2_leaf_reg"),
                                        ("learning_rate", float("inf"), ValueError, "learning_rate"), ("reserved", 1, ValueError, "reserved")]:
            q = _lib.BoostFitParamsC.from_buffer_copy(p)
            setattr(q, field, value)
            with pytest.raises(exc, match=text):
                raw(q=q)
        q = _lib.BoostFitParamsC.from_buffer_copy(p)
        q.n_trees, q.depth = 1 << 20, 8
        with pytest.raises(NotImplementedError, match="WDX_BOOST_FIT_MAX_WORKSPACE"):
            raw(q=q)
        with pytest.raises(NotImplementedError, match="WDX_BOOST_FIT_MAX_ROWS"):
            raw(n=(1 << 24) + 1)
        with pytest.raises(ValueError, match="ld = 4"):
            raw(ld=4)
        for kw, text in [(dict(Xp=None), "fingerprints are required"), (dict(yp=None), "class indices are required"), (dict(Sp=None), "scores are required"),
                         (dict(o=[out[0], None, out[2]]), "split_feature, split_border and leaf_values")]:
            with pytest.raises(ValueError, match=text):
                raw(**kw)
        ms, launches = eng.kernel_time(_lib.K_BOOST_FIT)
        assert launches == 0, launches
        # a class index outside 0 .. k-1 is found on the device before the first tree: nothing is written, and the timer has
        # counted the one kernel that ran (the binarisation, which makes the check), not the trees that did not
        for i, yy in enumerate((bad_y, neg_y)):
            with pytest.raises(ValueError, match="class index lies outside 0 .. 2"):
                fit(y_idx=yy, n_trees=3)
            assert eng.kernel_time(_lib.K_BOOST_FIT)[1] == i + 1
        assert not Sd.any().item()
    finally:
        eng.kernel_timing(False)
    after = [t.cpu().numpy() for t in eng.boost_predict(Xd, want_raw=True)]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    got = fit()
    ref, S_ref = rule.fit(X, y, 3, 1, 2, LR, LAM, 16)
    assert np.array_equal(got.split_feature[0], ref.split_feature[0]) and np.array_equal(Sd.cpu().numpy(), S_ref)


def test_kernel_time_counts_the_launches(eng):
    X, y = rule.synthetic(300, 8, 3, seed=1)
    eng.kernel_timing(True)
    try:
        eng.kernel_time_reset()
        device_fit(eng, X, y, 3, 4, 3, 16)
        ms, launches = eng.kernel_time(_lib.K_BOOST_FIT)
    finally:
        eng.kernel_timing(False)
    assert launches == 1 + 4 * (3 * 3 + 4) == 53 and ms > 0, (ms, launches)   # binarise + 4 trees of (gradient, 3 x 3 levels, 3 for the leaves)


# ---- learning --------------------------------------------------------------------------------------------------------------------------

def test_held_out_accuracy_equals_the_restatements():
    """4 classes, templates plus noise: chance is 1/4.  The predictions follow from the bits; asserted through `predict`."""
    _imports()
    X, y = rule.synthetic(3000, 25, 4, seed=17)
    Xtr, ytr, Xte, yte = X[:2000], y[:2000], X[2000:], y[2000:]
    m = models.Fpt_Boost.fit(Xtr, ytr, n_trees=30, depth=4, learning_rate=LR, l2_leaf_reg=LAM, border_count=32)
    ref, _ = rule.fit(Xtr, ytr, 4, 30, 4, LR, LAM, 32)
    raw_ref = boost_ref.raw_scores(ref.model(25), Xte)
    pred, _ = m.predict(Xte)
    acc, acc_ref = float((pred == yte).mean()), float((np.argmax(raw_ref, axis=1) == yte).mean())
    print(f"held-out accuracy: device {acc:.4f}, restatement {acc_ref:.4f}")
    assert np.array_equal(m.predict_raw(Xte)[0], raw_ref)
    assert acc == acc_ref and acc > 0.5
