"""Cross-validated probabilities on the device (DemuxEngine.svm_cross_val, include/wdx.h: wdx_svm_cv_couple_device;
models.DTW_SVM.cross_val_predict, DTW_SVM.fit(thresholds="cv")).

  * the one launch: on the DOWNLOADED device kernel matrix, alpha / rho / n_iter / state / dec of every problem of the plan are
    the bits of tests/helpers/svm_fit_rule.py's solver on the same batch -- m = 120, k = 4, cv = 5 (180 problems); m = 200,
    k = 10, cv = 2; k = 2; with the full data's own problems behind the folds', whose model is `_svm_fit.fit_arrays` on that K;
  * the coupling kernel alone, on planted decision values: probabilities against tests/helpers/svm_ref.py's
    multiclass_probability at 1e-12 on the rows beyond tests/test_gpu_svm.py's stopping margin (that file's exact tier); the
    class index and the margin are exactly the first maximum and top1 - top2 of the device's own probabilities, and the index
    is the helper's where its margin exceeds 1e-9; k = 2, 3, 10, 16; folds that hold out 1, 3, 4, 5 and 257 rows (partial
    groups of four, more than one workgroup); NaN decision values;
  * a NaN planted in K where only fold 0's problems read it: fold 0's rows come back NaN / -1, the others keep their bits;
  * the deployed tail: the model of fold f's arrays predicts X[H_f] through DTW_SVM.predict; the probabilities agree with the
    out-of-fold ones at 1e-5 beyond the stopping margin of 1e-5 (the float32 tier of tests/test_gpu_svm.py: the tail's kernel
    values come from expf, the training matrix's from exp_rule);
  * end to end: fit(thresholds="cv") on 10 classes x 60 fingerprints with 15 % of the labels swapped.
"""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import svm_fit_rule as rule  # noqa: E402
from helpers import svm_ref  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN_EXACT = 1e-8     # tests/test_gpu_svm.py: the stopping-margin rule of its exact tier ...
MARGIN_FLOAT32 = 1e-5   # ... and of comparisons whose kernel values may differ by a float32 ulp
L, WINDOW, PENALTY = 25, 15, 0.1


def _imports():
    global torch, _lib, _svm_cv, _svm_fit, DemuxEngine, DTW_SVM
    import torch
    from warpdemux_amd import _lib, _svm_cv, _svm_fit
    from warpdemux_amd.engine import DemuxEngine
    from warpdemux_amd.models import DTW_SVM


@pytest.fixture(scope="module")
def eng():
    _imports()
    e = DemuxEngine(np.zeros((4, L)), WINDOW, PENALTY)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _fingerprints(counts, seed, noise=0.8, swap=0.0):
    """(X float64 (m, L), y): noisy copies of one random prototype per class, shuffled; ``swap``: the share of labels replaced"""
    rng = np.random.default_rng(seed)
    k = len(counts)
    proto = rng.normal(size=(k, L))
    y = rng.permutation(np.repeat(np.arange(k), counts))
    X = proto[y] + noise * rng.normal(size=(len(y), L))
    lab = y.copy()
    sw = rng.random(len(y)) < swap
    lab[sw] = rng.integers(0, k, int(sw.sum()))
    return np.ascontiguousarray(X), lab


def _device_kernel(eng, X, gamma=0.05):
    D = eng.self_distances(torch.tensor(X, device="cuda"), WINDOW, PENALTY)
    return eng.svm_kernel(D, gamma, 1, out=D)


@pytest.mark.parametrize("counts,cv,with_full", [((40, 35, 25, 20), 5, False), ((20,) * 10, 2, False), ((33, 27), 3, True), ((40, 35, 25, 20), 5, True)])
def test_one_launch_equals_the_restated_solver_on_the_planned_batch(eng, counts, cv, with_full):
    X, y = _fingerprints(counts, seed=len(counts) + cv)
    k = len(counts)
    K = _device_kernel(eng, X)
    res = eng.svm_cross_val(K, y, k, C=1.0, class_weight="balanced", tol=1e-3, random_state=4, cv=cv, with_full=with_full)
    Kh = np.ascontiguousarray(K.cpu().numpy())
    p = res.plan
    n_pairs = k * (k - 1) // 2
    assert len(p.batch.problems) == (cv + with_full) * n_pairs * 6
    want = rule.solve_batch(Kh, p.batch, 1e-3, rule.default_max_iter(0))
    for name in ("alpha", "rho", "n_iter", "state", "dec"):
        assert np.array_equal(getattr(res.solution, name), getattr(want, name)), name
    assert (want.state == 0).all()
    assert np.array_equal(res.fold_of_row, _svm_cv.outer_folds(y, k, cv, 4)[0])
    if with_full:
        w = _svm_fit.class_weights("balanced", np.arange(k), y)
        full = _svm_fit.fit_arrays(Kh, y, k, 1.0 * w, 1e-3, -1, 4, rule.solve_batch)
        for a, b in zip(res.full, full[:6]):
            assert np.array_equal(a, b)
    # every row is held out once and has probabilities
    prob = res.prob.cpu().numpy()
    assert np.isfinite(prob).all() and np.allclose(prob.sum(axis=1), 1.0, atol=1e-12)
    assert (res.pred_idx.cpu().numpy() == np.argmax(prob, axis=1)).all()


def _couple_reference(dec, A, B, k):
    """(prob, stopping margin) of rows of decision values (n, pairs): sigmoid_predict, the clamp, multiclass_probability"""
    fApB = dec * A[None, :] + B[None, :]
    with np.errstate(over="ignore"):
        e_neg, e_pos = np.exp(-fApB), np.exp(fApB)
        sig = np.where(fApB >= 0, e_neg / (1.0 + e_neg), 1.0 / (1.0 + e_pos))
    v = np.minimum(np.maximum(sig, svm_ref.MIN_PROB), 1 - svm_ref.MIN_PROB)
    r = np.zeros((len(dec), k, k))
    for q, (i, j) in enumerate(svm_ref._pairs(k)):
        r[:, i, j] = v[:, q]
        r[:, j, i] = 1 - v[:, q]
    prob, margin, _ = svm_ref._multiclass_probability(r)
    return prob, margin


def _couple(eng, dec, off, A, B, held, held_off, m, k):
    d = torch.tensor(dec, device="cuda")
    prob = torch.full((m, k), -5.0, dtype=torch.float64, device="cuda")
    pred = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    conf = torch.full((m,), -5.0, dtype=torch.float64, device="cuda")
    rc = eng.L.wdx_svm_cv_couple_device(eng.ctx.handle, d.data_ptr(), len(dec), k, len(held_off) - 1, off.ctypes.data, A.ctypes.data, B.ctypes.data,
                                     held.ctypes.data, held_off.ctypes.data, m, prob.data_ptr(), pred.data_ptr(), conf.data_ptr(), eng._stream())
    return rc, prob.cpu().numpy(), pred.cpu().numpy(), conf.cpu().numpy()


@pytest.mark.parametrize("k", [2, 3, 10, 16])
def test_coupling_kernel_on_planted_decision_values(eng, k):
    rng = np.random.default_rng(100 + k)
    counts = [1, 3, 4, 5, 257]
    F, n_pairs, total = len(counts), k * (k - 1) // 2, sum(counts)
    m = total + 13
    held = rng.permutation(m)[:total].astype(np.int32)                     # 13 rows are in no fold
    held_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    A = -rng.uniform(0.3, 4.0, size=(F, n_pairs))
    B = rng.normal(0.0, 0.5, size=(F, n_pairs))
    # every (fold, pair) block somewhere of its own in dec, in a shuffled order with gaps between the blocks
    off = np.zeros((F, n_pairs), np.int64)
    at = 3
    for c in rng.permutation(F * n_pairs):
        off[c // n_pairs, c % n_pairs] = at
        at += counts[c // n_pairs] + int(rng.integers(0, 5))
    dec = rng.normal(0.0, 1.5, size=at + 2)
    dec[rng.permutation(at)[: at // 20]] *= 40.0                            # both clips and both sigmoid branches
    rc, prob, pred, conf = _couple(eng, dec, off, A, B, held, held_off, m, k)
    assert rc == 0
    untouched = np.setdiff1d(np.arange(m), held)
    assert (prob[untouched] == -5.0).all() and (pred[untouched] == -7).all() and (conf[untouched] == -5.0).all()
    n_use = 0
    for f in range(F):
        H = held[held_off[f]: held_off[f + 1]]
        rows = np.stack([dec[off[f, q]: off[f, q] + counts[f]] for q in range(n_pairs)], axis=1)
        want, margin = _couple_reference(rows, A[f], B[f], k)
        use = margin >= MARGIN_EXACT
        n_use += int(use.sum())
        np.testing.assert_allclose(prob[H][use], want[use], rtol=0, atol=1e-12)
        srt = np.sort(want, axis=1)
        np.testing.assert_allclose(conf[H][use], (srt[:, -1] - srt[:, -2])[use], rtol=0, atol=1e-12)
        far = use & (srt[:, -1] - srt[:, -2] > 1e-9)
        assert np.array_equal(pred[H][far], np.argmax(want, axis=1)[far])
        own = np.sort(prob[H], axis=1)
        assert np.array_equal(pred[H], np.argmax(prob[H], axis=1)) and np.array_equal(conf[H], own[:, -1] - own[:, -2])
    assert n_use >= 0.97 * total
    # NaN decision values: those rows NaN / -1, every other row keeps its bits
    dec2 = dec.copy()
    hit_rows = [(4, 0, 5), (4, n_pairs - 1, 256), (1, 0, 2)]                # (fold, pair, entry)
    for f, q, e in hit_rows:
        dec2[off[f, q] + e] = np.nan
    rc, prob2, pred2, conf2 = _couple(eng, dec2, off, A, B, held, held_off, m, k)
    bad = np.array([held[held_off[f] + e] for f, _, e in hit_rows])
    assert rc == 0 and np.isnan(prob2[bad]).all() and (pred2[bad] == -1).all() and np.isnan(conf2[bad]).all()
    rest = np.setdiff1d(np.arange(m), bad)
    assert np.array_equal(prob2[rest], prob[rest]) and np.array_equal(pred2[rest], pred[rest]) and np.array_equal(conf2[rest], conf[rest])


def test_coupling_entry_refuses_bad_tables_and_the_context_stays_usable(eng):
    k, F = 3, 2
    held, held_off = np.array([0, 1, 2], np.int32), np.array([0, 1, 3], np.int64)
    off = np.array([[0, 1, 2], [3, 5, 7]], np.int64)
    A, B, dec = -np.ones((F, 3)), np.zeros((F, 3)), np.linspace(-1, 1, 9)
    ok = _couple(eng, dec, off, A, B, held, held_off, 3, k)
    assert ok[0] == 0 and np.isfinite(ok[1]).all()
    cases = [dict(k=1), dict(k=17), dict(m=2), dict(off=np.array([[0, 1, 2], [3, 5, 8]], np.int64)), dict(off=np.array([[0, 1, -1], [3, 5, 7]], np.int64)),
             dict(held_off=np.array([1, 1, 3], np.int64)), dict(held_off=np.array([0, 2, 1], np.int64)), dict(held=np.array([0, 1, 3], np.int32)),
             dict(held=np.array([0, -1, 2], np.int32))]
    for c in cases:
        a = dict(dec=dec, off=off, A=A, B=B, held=held, held_off=held_off, m=3, k=k)
        a.update(c)
        assert _couple(eng, **a)[0] == _lib.WDX_ERR_INVALID, c
    again = _couple(eng, dec, off, A, B, held, held_off, 3, k)
    assert again[0] == 0 and np.array_equal(again[1], ok[1])


def test_a_nan_in_the_kernel_matrix_ends_one_folds_problem_and_leaves_the_other_fold_alone(eng):
    X, y = _fingerprints((30, 26), seed=8)
    K = _device_kernel(eng, X)
    clean = eng.svm_cross_val(K, y, 2, random_state=1, cv=2)
    # two rows of fold 0's TRAINING part (both held out by fold 1): only fold 0's problems ever read K[a, b]
    a, b = clean.held[1][:2]
    K2 = K.clone()
    K2[a, b] = float("nan")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = eng.svm_cross_val(K2, y, 2, random_state=1, cv=2)
    full0 = (got.fit_info["part"] == 0) & (got.fit_info["fold"] == -1)
    assert got.fit_info["state"][full0].tolist() == [2] and (got.fit_info["state"][got.fit_info["part"] == 1] == 0).all()
    prob, pred, conf = got.prob.cpu().numpy(), got.pred_idx.cpu().numpy(), got.conf.cpu().numpy()
    H0, H1 = clean.held[0], clean.held[1]
    assert np.isnan(prob[H0]).all() and (pred[H0] == -1).all() and np.isnan(conf[H0]).all()
    assert np.array_equal(prob[H1], clean.prob.cpu().numpy()[H1]) and np.array_equal(pred[H1], clean.pred_idx.cpu().numpy()[H1])
    assert np.array_equal(conf[H1], clean.conf.cpu().numpy()[H1])


def test_out_of_fold_probabilities_agree_with_the_deployed_tail(eng):
    X, y = _fingerprints((40, 35, 25, 20), seed=21)
    gamma = 0.05
    K = _device_kernel(eng, X, gamma)
    res = eng.svm_cross_val(K, y, 4, class_weight="balanced", random_state=2, cv=5)
    prob = res.prob.cpu().numpy()
    Kh = K.cpu().numpy()
    for f in (0, 3):
        T, H = res.train[f], res.held[f]
        n_support, support, dual, rho, probA, probB = res.folds[f]
        model = DTW_SVM(X[T], n_support, support, dual, rho, probA, probB, {i: i for i in range(4)}, None, WINDOW, PENALTY, gamma=gamma)
        _, tail = model.predict(X[H], nproc=1)
        ref = svm_ref.predict(Kh[H][:, T], n_support, support, dual, rho, probA, probB)
        use = ref.margin >= MARGIN_FLOAT32
        assert use.mean() > 0.9
        np.testing.assert_allclose(prob[H][use], tail[use], rtol=0, atol=1e-5)


def test_fit_with_cross_validated_thresholds_end_to_end():
    _imports()
    X, y = _fingerprints((60,) * 10, seed=33, noise=1.0, swap=0.15)
    labels = 3 + 2 * y
    args = dict(window=WINDOW, penalty=PENALTY, gamma=0.05, C=1.0, class_weight="balanced", random_state=5)
    with pytest.raises(ValueError):
        DTW_SVM.fit(X, labels, thresholds="cv", solver="libsvm", **args)
    with pytest.raises(ValueError):
        DTW_SVM.fit(X, labels, thresholds="cv", solver="device", target_accuracy=0.9995, **args)
    with pytest.raises(ValueError):
        DTW_SVM.fit(X, labels, thresholds="cv", solver="device", cv=61, **args)
    model = DTW_SVM.fit(X, labels, thresholds="cv", solver="device", target_accuracy=0.95, cv=5, **args)
    thr = model.thresholds
    assert thr.shape == (10,) and not np.isnan(thr).any() and (thr >= 0.01).all() and np.array_equal(thr, model.cv_["thresholds"][0])
    y_pred, y_prob = model.predict(X, nproc=1)
    srt = np.sort(y_prob, axis=1)
    margin = srt[:, -1] - srt[:, -2]
    best = np.argmax(y_prob, axis=1)
    assert np.array_equal(y_pred == -1, margin < thr[best])       # (top1 - top2 of the same two float64 values: the tail's own margin)
    assert np.array_equal(y_pred[(y_pred != -1)], (3 + 2 * best)[y_pred != -1])
    cvp = DTW_SVM.cross_val_predict(X, labels, cv=5, **args)
    for key, v in zip(("prob", "pred", "conf", "fold"), cvp):
        assert np.array_equal(model.cv_[key], v, equal_nan=True), key
    assert set(np.unique(cvp[1]).tolist()) <= set((3 + 2 * np.arange(10)).tolist()) | {-1} and cvp[0].shape == (600, 10)
    kept, hit = model.cv_["kept"], model.cv_["hit"]
    assert kept.shape == (10, 101) and int(kept[:, 0].sum()) + model.cv_["skipped"] == 600 and (hit <= kept).all()
