"""models.DTW_SVM.fit and from_sklearn without a GPU: ``fit(distances=...)`` takes the training matrix from the caller -- here the
CPU oracle's -- and touches no device.  5 classes x 300 rows, L 25, window 15, penalty 0.1 (the shipped models' shape), drawn as
tests/test_gpu_live.py's _svm_model draws its training set."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import wdx_oracle as orc  # noqa: E402
from helpers import self_matrix_rule as sr  # noqa: E402

K_CLASSES, N_TRAIN, L, WINDOW, PENALTY = 5, 300, 25, 15, 0.1
LABELS = np.array([3, 7, 11, 12, 40])   # non-contiguous barcode numbers


@pytest.fixture(scope="module")
def data():
    Xtr, y, _, _ = sr.training_rows(K_CLASSES, N_TRAIN, L, seed=3)
    D = orc.dtw_matrix(Xtr, Xtr, WINDOW, PENALTY)
    D.setflags(write=False)
    return Xtr, y, D


def _kernel(D, gamma=1.0, pwr_dist=1):
    """the reference's pdist_kernel (models/dtw_svm.py), on the float32 matrix as it is"""
    return np.exp(-gamma * np.power(D, pwr_dist))


def _svc(K, y, **kw):
    from sklearn.svm import SVC

    return SVC(kernel="precomputed", probability=True, random_state=0, **kw).fit(K, y)


def _same_model(model, svc):
    want = orc.svm_params(svc)
    got = (model._n_support, model._support, model._dual_coef, model._rho, model._probA, model._probB)
    for name, g, w in zip(("n_support", "support", "dual_coef", "rho", "probA", "probB"), got, want[:6]):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name
    assert model.n_classes == want[6]


def test_fit_on_given_distances_equals_an_svc_on_the_same_kernel(data):
    from warpdemux_amd.models import DTW_SVM

    Xtr, y, D = data
    model = DTW_SVM.fit(Xtr, y, WINDOW, PENALTY, distances=D)
    svc = _svc(_kernel(D), y)
    _same_model(model, svc)
    assert model.n_dropped_ == 0 and model.window == WINDOW and model.penalty == PENALTY and model.gamma == 1.0 and model.pwr_dist == 1
    assert model.label_mapper == {i: i for i in range(K_CLASSES)} and model.thresholds is None
    assert model._X.dtype == np.float64 and np.array_equal(model._X, Xtr)
    # gamma, pwr_dist and C reach the kernel and the estimator; thresholds reach the model
    thr = np.full(K_CLASSES, 0.2)
    m2 = DTW_SVM.fit(Xtr, y, WINDOW, PENALTY, gamma=0.5, pwr_dist=2, C=3.0, thresholds=thr, distances=D, block_size=500)
    _same_model(m2, _svc(_kernel(D, 0.5, 2), y, C=3.0))
    assert m2.gamma == 0.5 and m2.pwr_dist == 2 and np.array_equal(m2.thresholds, thr) and m2.block_size == 500
    assert not np.array_equal(m2._dual_coef, model._dual_coef) or m2._dual_coef.shape != model._dual_coef.shape


def test_label_mapper_follows_classes_for_non_contiguous_labels(data):
    from warpdemux_amd.models import DTW_SVM

    Xtr, y, D = data
    model = DTW_SVM.fit(Xtr, LABELS[y], WINDOW, PENALTY, distances=D)
    assert model.label_mapper == {i: int(c) for i, c in enumerate(LABELS)}
    assert model._label_arr.tolist() == LABELS.tolist()
    _same_model(model, _svc(_kernel(D), LABELS[y]))


def test_a_nan_row_and_a_status_row_are_dropped_and_counted(data):
    from warpdemux_amd.models import DTW_SVM

    Xtr, y, D = data
    X = Xtr.copy()
    X[17, 4] = np.nan
    X[120, 24] = np.inf
    status = np.zeros(N_TRAIN, dtype=np.int32)
    status[203] = 1
    keep = np.ones(N_TRAIN, dtype=bool)
    keep[[17, 120, 203]] = False
    Dm = np.ascontiguousarray(D[np.ix_(keep, keep)])
    model = DTW_SVM.fit(X, y, WINDOW, PENALTY, status=status, distances=Dm)
    assert model.n_dropped_ == 3 and model._X.shape == (N_TRAIN - 3, L) and np.array_equal(model._X, Xtr[keep])
    _same_model(model, _svc(_kernel(Dm), y[keep]))
    with pytest.raises(ValueError, match=r"distances must be the \(297, 297\) matrix of the 297 members"):
        DTW_SVM.fit(X, y, WINDOW, PENALTY, status=status, distances=D)


def test_the_value_errors_fire_before_any_device_work(data, monkeypatch):
    from warpdemux_amd import _lib
    from warpdemux_amd.models import DTW_SVM

    def no_device(*a, **k):
        raise AssertionError("fit touched the device before it refused")

    monkeypatch.setattr(_lib, "default_context", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    Xtr, y, D = data
    with pytest.raises(ValueError, match="at least two classes among the members, found 1"):
        DTW_SVM.fit(Xtr, np.zeros(N_TRAIN, dtype=np.int64), WINDOW, PENALTY)
    one_left = np.where(y == 0, 0, 1)
    st = (one_left == 1).astype(np.int32)     # every row of the second class has status 1
    with pytest.raises(ValueError, match="at least two classes among the members, found 1"):
        DTW_SVM.fit(Xtr, one_left, WINDOW, PENALTY, status=st)
    with pytest.raises(ValueError, match="17 classes: the resident SVM tail serves at most 16"):
        DTW_SVM.fit(Xtr, np.arange(N_TRAIN) % 17, WINDOW, PENALTY)
    with pytest.raises(ValueError, match=r"y must hold one label per row: shape \(300,\), not \(299,\)"):
        DTW_SVM.fit(Xtr, y[:-1], WINDOW, PENALTY)
    with pytest.raises(ValueError, match=r"y must hold one label per row"):
        DTW_SVM.fit(Xtr, y.reshape(-1, 1), WINDOW, PENALTY)
    with pytest.raises(ValueError, match=r"status must hold one value per row: shape \(300,\), not \(10,\)"):
        DTW_SVM.fit(Xtr, y, WINDOW, PENALTY, status=np.zeros(10, dtype=np.int32))
    with pytest.raises(ValueError, match=r"distances must be the \(300, 300\) matrix"):
        DTW_SVM.fit(Xtr, y, WINDOW, PENALTY, distances=D[:, :299])
    with pytest.raises(ValueError, match=r"distances must be the \(300, 300\) matrix"):
        DTW_SVM.fit(Xtr, y, WINDOW, PENALTY, distances=D.ravel())
    # 16 classes are served
    assert DTW_SVM.fit(Xtr, np.arange(N_TRAIN) % 16, WINDOW, PENALTY, distances=D).n_classes == 16


def test_from_sklearn_is_the_extraction_from_reference_does(data):
    from warpdemux_amd.models import DTW_SVM

    Xtr, y, D = data
    svc = _svc(_kernel(D), y)
    thr = np.full(K_CLASSES, 0.3)
    a = DTW_SVM.from_sklearn(svc, Xtr, {i: i + 1 for i in range(K_CLASSES)}, thr, WINDOW, PENALTY, gamma=1.0, pwr_dist=1, block_size=500)

    class Reference:   # the attributes of the reference's DTW_SVM that from_reference reads
        model, _X, label_mapper, thresholds, window, penalty, gamma, pwr_dist, block_size = (
            svc, Xtr, {i: i + 1 for i in range(K_CLASSES)}, thr, WINDOW, PENALTY, 1.0, 1, 500)

    b = DTW_SVM.from_reference(Reference())
    _same_model(a, svc), _same_model(b, svc)
    assert a.label_mapper == b.label_mapper and np.array_equal(a.thresholds, b.thresholds) and a.block_size == b.block_size == 500
    from sklearn.svm import SVC

    with pytest.raises(ValueError, match="expected SVC"):
        DTW_SVM.from_sklearn(SVC(kernel="rbf", probability=True), Xtr, {}, None, WINDOW, PENALTY)
