"""Accuracy thresholds on the device (include/wdx.h: wdx_accuracy_thresholds_device, wdx_accuracy_thresholds;
DemuxEngine.accuracy_thresholds; models.accuracy_thresholds) against the rule restated in NumPy (warpdemux_amd/_thresholds.py:
rule, itself held to a sort-based brute force by tests/test_thresholds_host.py): thresholds, kept, hit and skipped bit for bit.

Shapes: n = 1, 63 / 64 / 65 (a wave), 4 097 (one row more than a workgroup's 4 096) and 70 000 (18 workgroups that flush into
the same counters); k = 2, 10, 16; R = 1, 100, 1 000 (the 16 classes take two groups of LDS counters) and 4 096 (one class per
group).  Margins exactly on i / R, one ulp either side, 0 and 1; rows with NaN / inf probabilities and y_idx = -1; a class
never predicted; targets 0, 950, 999 and 1000."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TARGETS = (0.0, 0.95, 0.999, 1.0)
PM = np.array([0, 950, 999, 1000], np.int32)


def _imports():
    global torch, _lib, _thresholds, DemuxEngine, models
    import torch
    from warpdemux_amd import _lib, _thresholds, models
    from warpdemux_amd.engine import DemuxEngine


@pytest.fixture(scope="module")
def eng():
    _imports()
    e = DemuxEngine(np.random.default_rng(0).normal(size=(4, 25)), 15, 0.1)
    yield e
    e.close()


def _case(n, k, R, seed):
    """softmax rows of noisy labels; class k - 1 is never predicted; the first rows carry margins on and next to grid values"""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, k - 1, n).astype(np.int32)
    logits = rng.normal(size=(n, k)) + 2.5 * (np.arange(k)[None, :] == y[:, None])
    logits[:, k - 1] = -30.0
    swap = rng.random(n) < 0.2
    y[swap] = rng.integers(0, k, int(swap.sum()))
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    prob = e / e.sum(axis=1, keepdims=True)
    grid = np.arange(R + 1, dtype=np.float64) / np.float64(R)
    edge = []
    for g in grid[rng.permutation(R + 1)[:40]].tolist() + [0.0, 1.0]:
        edge += [g, float(np.nextafter(g, 0.0)) if g > 0 else 0.0, float(np.nextafter(g, 2.0))]
    for r, conf in zip(range(8, n), edge):
        prob[r] = 0.0
        prob[r, r % (k - 1)] = conf                 # top1 - top2 = conf - 0 exactly
    if n > 7:
        prob[1, 0], prob[2, k - 1], prob[3, 1] = np.nan, np.inf, -np.inf
        y[4] = -1
        prob[5] = 1.0 / k                           # a tie: the first maximum, margin 0
    return np.ascontiguousarray(prob), y


def _check(eng, prob, y, R):
    want = _thresholds.rule(prob, y, PM, R)
    dp, dy = torch.tensor(prob, device="cuda"), torch.tensor(y, device="cuda")
    got = [t.cpu().numpy() for t in eng.accuracy_thresholds(dp, dy, TARGETS, R)]
    for g, w, name in zip(got, want, ("thr", "kept", "hit", "skipped")):
        assert np.array_equal(g, w), name
    again = [t.cpu().numpy() for t in eng.accuracy_thresholds(dp, dy, TARGETS, R)]
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 70000])
def test_rows_across_waves_workgroups_and_flushes(eng, n):
    prob, y = _case(n, 10, 100, seed=n)
    thr = _check(eng, prob, y, 100)[0]
    if n >= 4097:
        assert np.isinf(thr[:, 9]).all() and np.isfinite(thr[0, :9]).all()     # the class never predicted; target 0 is reachable
        assert (thr[1:] >= thr[:-1]).all()


@pytest.mark.parametrize("k", [2, 10, 16])
@pytest.mark.parametrize("R", [1, 100, 1000, 4096])
def test_classes_and_resolutions(eng, k, R):
    prob, y = _case(5000, k, R, seed=31 * k + R)
    _check(eng, prob, y, R)


def test_host_form_and_the_generic_door(eng):
    prob, y = _case(3000, 10, 100, seed=5)
    want = _thresholds.rule(prob, y, PM, 100)
    got = _thresholds.host(prob, y, PM, 100)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    empty = _thresholds.host(np.zeros((0, 4)), np.zeros(0, np.int32), PM, 100)
    assert np.isinf(empty[0]).all() and empty[1].sum() == 0 and empty[3] == 0
    mapper = {i: 10 + 2 * i for i in range(10)}
    labels = np.where(y >= 0, 10 + 2 * y, -1)
    table = models.accuracy_thresholds(prob, labels, mapper, TARGETS)
    assert np.array_equal(table, want[0])
    one = models.accuracy_thresholds(prob, labels, mapper, 0.95)
    assert one.shape == (10,) and np.array_equal(one, want[0][1])
    with pytest.raises(ValueError):
        models.accuracy_thresholds(prob, labels, mapper, 0.9995)
    with pytest.raises(ValueError):
        models.accuracy_thresholds(prob, labels, {i: i for i in range(9)}, 0.95)


def test_thresholds_straight_from_the_svm_tail_output(eng, golden_dir):
    """device probabilities of `svm_predict` go in as they are"""
    from warpdemux_amd.models import DTW_SVM

    z = np.load(os.path.join(golden_dir, "g6_dtw_svm_wdx4.npz"))
    mapper = {int(i): int(c) for i, c in zip(z["label_keys"], z["label_vals"])}
    k = len(z["n_support"])
    m = DTW_SVM(z["X_train"], z["n_support"], z["support"], z["dual_coef"], -z["intercept"], z["probA"], z["probB"], mapper, None,
                int(z["window"]), float(z["penalty"]), gamma=float(z["gamma"]), pwr_dist=int(z["pwr_dist"]))
    eng.set_refs(z["X_train"], int(z["window"]), float(z["penalty"]))
    eng.set_svm(m)
    X = torch.tensor(np.ascontiguousarray(z["Xq"]), device="cuda")
    prob, pred, conf = eng.svm_predict(eng.dtw(X, want_argmin=False)[0])
    y = torch.tensor(np.random.default_rng(1).integers(0, k, len(X)).astype(np.int32), device="cuda")
    thr, kept, hit, skipped = eng.accuracy_thresholds(prob, y, (0.5,), 100)
    want = _thresholds.rule(prob.cpu().numpy(), y.cpu().numpy(), [500], 100)
    assert np.array_equal(thr.cpu().numpy(), want[0]) and np.array_equal(kept.cpu().numpy(), want[1]) and int(skipped) == want[3]


def test_bad_arguments_are_refused_and_the_context_stays_usable(eng):
    prob, y = _case(100, 4, 100, seed=9)
    dp, dy = torch.tensor(prob, device="cuda"), torch.tensor(y, device="cuda")
    thr = torch.empty((1, 4), dtype=torch.float64, device="cuda")
    L, h, s = eng.L, eng.ctx.handle, eng._stream()
    pm = np.array([990], np.int32)
    P = lambda a: a.ctypes.data  # noqa: E731
    bad = [(dp.data_ptr(), 100, 1, dy.data_ptr(), 100, P(pm), 1, thr.data_ptr()), (dp.data_ptr(), 100, 17, dy.data_ptr(), 100, P(pm), 1, thr.data_ptr()),
           (dp.data_ptr(), 100, 4, dy.data_ptr(), 0, P(pm), 1, thr.data_ptr()), (dp.data_ptr(), 100, 4, dy.data_ptr(), 4097, P(pm), 1, thr.data_ptr()),
           (dp.data_ptr(), 100, 4, dy.data_ptr(), 100, P(pm), 0, thr.data_ptr()), (dp.data_ptr(), 100, 4, dy.data_ptr(), 100, P(pm), 17, thr.data_ptr()),
           (dp.data_ptr(), 100, 4, dy.data_ptr(), 100, None, 1, thr.data_ptr()), (dp.data_ptr(), 100, 4, dy.data_ptr(), 100, P(pm), 1, None),
           (None, 100, 4, dy.data_ptr(), 100, P(pm), 1, thr.data_ptr()), (dp.data_ptr(), 100, 4, None, 100, P(pm), 1, thr.data_ptr()),
           (dp.data_ptr(), -1, 4, dy.data_ptr(), 100, P(pm), 1, thr.data_ptr()),
           (dp.data_ptr(), 100, 4, dy.data_ptr(), 100, P(np.array([1001], np.int32)), 1, thr.data_ptr()),
           (dp.data_ptr(), 100, 4, dy.data_ptr(), 100, P(np.array([-1], np.int32)), 1, thr.data_ptr())]
    for a in bad:
        assert L.wdx_accuracy_thresholds_device(h, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], None, None, None, s) == _lib.WDX_ERR_INVALID, a
    for call in (lambda: eng.accuracy_thresholds(dp.float(), dy), lambda: eng.accuracy_thresholds(dp, dy.long()),
                 lambda: eng.accuracy_thresholds(dp, dy, (0.9995,)), lambda: eng.accuracy_thresholds(dp, dy, resolution=0),
                 lambda: eng.accuracy_thresholds(dp[:, :1].contiguous(), dy)):
        with pytest.raises(ValueError):
            call()
    # the outputs the caller does not want stay in the context; the thresholds are the same
    assert L.wdx_accuracy_thresholds_device(h, dp.data_ptr(), 100, 4, dy.data_ptr(), 100, P(pm), 1, thr.data_ptr(), None, None, None, s) == 0
    assert np.array_equal(thr.cpu().numpy(), _thresholds.rule(prob, y, pm, 100)[0])


def test_outputs_stay_inside_the_sizes_the_header_states(eng):
    """thr (T, k), kept and hit (k, R + 1) and the one skipped count between guard words that keep their values"""
    k, R = 16, 1000                                     # two groups of classes in pass one
    prob, y = _case(9000, k, R, seed=77)
    dp, dy = torch.tensor(prob, device="cuda"), torch.tensor(y, device="cuda")

    def guarded(n, dtype):
        t = torch.full((n + 16,), -3, dtype=dtype, device="cuda")
        return t, t[8: 8 + n]

    (gt, vt), (gk, vk), (gh, vh), (gs, vs) = (guarded(len(PM) * k, torch.float64), guarded(k * (R + 1), torch.int64),
                                              guarded(k * (R + 1), torch.int64), guarded(1, torch.int64))
    rc = eng.L.wdx_accuracy_thresholds_device(eng.ctx.handle, dp.data_ptr(), len(y), k, dy.data_ptr(), R, PM.ctypes.data, len(PM), vt.data_ptr(),
                                              vk.data_ptr(), vh.data_ptr(), vs.data_ptr(), eng._stream())
    assert rc == 0
    want = _thresholds.rule(prob, y, PM, R)
    assert np.array_equal(vt.cpu().numpy().reshape(len(PM), k), want[0]) and np.array_equal(vk.cpu().numpy().reshape(k, R + 1), want[1])
    assert np.array_equal(vh.cpu().numpy().reshape(k, R + 1), want[2]) and int(vs[0]) == want[3]
    for g in (gt, gk, gh, gs):
        assert (g[:8] == -3).all() and (g[-8:] == -3).all()
