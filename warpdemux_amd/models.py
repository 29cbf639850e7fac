"""MI355X counterparts of ``warpdemux.models.dtw_svm.DTW_SVM``, ``dtw_mlp.DTW_MLP`` and
``fpt_boost.Fpt_Boost`` (at the end of the file: oblivious trees on the fingerprints themselves, no DTW).

Same ``predict`` signature and outputs as the reference (/root/reference/warpdemux/models/dtw_svm.py:54-98):
DTW distances to ``_X`` -> ``exp(-gamma * d**pwr_dist)`` -> ``SVC.predict_proba`` -> ``process_probs``
(models/utils.py:45-61) -> optional DataFrame (models/utils.py:36-43), with the whole chain on the device
(the (nX, len(_X)) distance matrix never leaves HBM).  Build one from a loaded reference model with
``DTW_SVM.from_reference(model)`` -- the fitted scikit-learn ``SVC`` is only read for its parameters.
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Dict, Optional, Tuple, Union

import numpy as np

from . import _lib, _marshal


def predictions_to_df(y_pred, y_prob, conf, label_mapper):
    """models/utils.py:36-43"""
    import pandas as pd

    return pd.DataFrame(
        {
            "predicted_barcode": y_pred,
            "confidence_score": conf.round(3),
            **{f"p{label_mapper[i]:02d}": y_prob[:, i].round(4) for i in range(y_prob.shape[1])},
        }
    )


def _own_slot(ctx, model):
    """``model`` into its slot of ``ctx`` unless it is the one the context last received there (``model._owner_attr``); no
    owner is recorded while the upload runs, so a refused model does not pass for the resident one."""
    if getattr(ctx, model._owner_attr, None) is not model:
        setattr(ctx, model._owner_attr, None)
        _marshal.set_model(ctx, model)
        setattr(ctx, model._owner_attr, model)
    return ctx


class _ResidentDTWModel:
    """What DTW_SVM and DTW_MLP share: the reference fingerprints, the DTW parameters and the label map on the host, the
    upload to the process's context, and ``predict``'s validation.  Subclasses name their context slot (``_owner_attr``)
    and the text of the column-mismatch error (``_column_error``)."""

    _owner_attr: str

    def _init_common(self, _X, window, penalty, block_size, label_mapper, thresholds, device):
        self._X = np.ascontiguousarray(_X, dtype=np.float64)
        self.window, self.penalty, self.block_size = window, penalty, block_size
        self.label_mapper = dict(label_mapper)
        self.thresholds = None if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64)
        self._device = device

    @property
    def is_trained(self):
        return self._X is not None

    def _ensure_resident(self):
        """References and model parameters on the process's context.  The context holds ONE reference set and ONE
        model per slot (the SVM's and the MLP's are separate) at a time and other calls (distance_matrix_to,
        set_references, another model of the same class) may have replaced either: the reference set is re-submitted on
        every call (the library compares a content hash and uploads only on change), the model whenever this object is
        not the one the context last received."""
        ctx = _lib.default_context(self._device)
        _marshal.set_refs(ctx, self._X, self.window, self.penalty)
        return _own_slot(ctx, self)

    def _predict_inputs(self, X, nproc, block_size, k):
        """``predict``'s prologue: (context, contiguous float64 X, y_prob (n, k), y_pred int32 (n,), conf (n,))."""
        if not self.is_trained:
            msg = "Model not trained yet."
            logging.error(msg)
            raise ValueError(msg)
        X = np.asarray(X)
        if X.ndim == 1:
            X = X.reshape(1, -1)
        if X.shape[1] != self._X.shape[1]:
            raise ValueError(self._column_error())
        if nproc != 1 and (self.block_size if block_size is None else block_size) is None:
            msg = "block_size must be specified when using parallel."
            logging.error(msg)
            raise ValueError(msg)
        X = np.ascontiguousarray(X, dtype=np.float64)
        n = X.shape[0]
        ctx = self._ensure_resident()
        return ctx, X, np.empty((n, k), dtype=np.float64), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64)


class DTW_SVM(_ResidentDTWModel):
    """Holds the reference fingerprints and the SVC parameters resident on one GPU context."""

    _owner_attr = "_svm_owner"

    def __init__(self, _X: np.ndarray, n_support, support, dual_coef, rho, probA, probB,
                 label_mapper: Dict[int, int], thresholds: Optional[np.ndarray], window: int, penalty: float,
                 gamma: float = 1.0, pwr_dist: int = 1, block_size: Optional[int] = None, device: Optional[int] = None):
        self._init_common(_X, window, penalty, block_size, label_mapper, thresholds, device)
        self.gamma, self.pwr_dist = float(gamma), int(pwr_dist)
        self._n_support = np.ascontiguousarray(n_support, dtype=np.int32)
        self._support = np.ascontiguousarray(support, dtype=np.int32)
        self._dual_coef = np.ascontiguousarray(dual_coef, dtype=np.float64)
        self._rho = np.ascontiguousarray(rho, dtype=np.float64)
        self._probA = np.ascontiguousarray(probA, dtype=np.float64)
        self._probB = np.ascontiguousarray(probB, dtype=np.float64)
        self.n_classes = int(self._n_support.size)
        self._label_arr = np.array([self.label_mapper[i] for i in range(self.n_classes)], dtype=np.int32)

    @classmethod
    def from_sklearn(cls, svc, _X, label_mapper, thresholds, window, penalty, gamma=1.0, pwr_dist=1,
                     block_size: Optional[int] = None, device: Optional[int] = None) -> "DTW_SVM":
        """From a fitted ``SVC(kernel="precomputed", probability=True)`` and the training fingerprints ``_X`` its kernel
        matrix was computed on: the estimator is only read for libsvm's parameters (``_n_support``, ``support_``,
        ``_dual_coef_``, ``-_intercept_``, ``_probA``, ``_probB``)."""
        if getattr(svc, "kernel", None) != "precomputed" or not getattr(svc, "probability", False):
            raise ValueError("expected SVC(kernel='precomputed', probability=True)")
        return cls(
            _X=_X, n_support=svc._n_support, support=svc.support_, dual_coef=svc._dual_coef_,
            rho=-np.asarray(svc._intercept_, dtype=np.float64), probA=svc._probA, probB=svc._probB,
            label_mapper=label_mapper, thresholds=thresholds, window=window, penalty=penalty, gamma=gamma,
            pwr_dist=pwr_dist, block_size=block_size, device=device,
        )

    @classmethod
    def from_reference(cls, model, device: Optional[int] = None) -> "DTW_SVM":
        """From a reference ``DTW_SVM`` instance (a loaded model_files/*.joblib)."""
        return cls.from_sklearn(model.model, model._X, model.label_mapper, model.thresholds, model.window, model.penalty,
                                gamma=model.gamma, pwr_dist=model.pwr_dist, block_size=model.block_size, device=device)

    @classmethod
    def fit(cls, X, y, window, penalty, gamma=1.0, pwr_dist=1, C=1.0, thresholds=None, status=None, distances=None,
            random_state=0, block_size: Optional[int] = None, device: Optional[int] = None, class_weight=None, solver="libsvm",
            tol=1e-3, max_iter=-1, target_accuracy=0.99, cv=5) -> "DTW_SVM":
        """Train a model on labelled fingerprints ``X`` (n, L), ``y`` (n,) integer barcode labels -- what the reference's
        training does (models/dtw_svm.py: ``pdist_kernel`` on the training set's own distance matrix, then a precomputed-kernel
        ``SVC`` with probabilities), with the matrix from the engine's symmetric self-distance kernels.

        1. members only: a row with a sample that is not finite, or whose ``status`` (optional, one integer per row) is not 0,
           is dropped; their number is ``n_dropped_`` of the returned model;
        2. ``D = parallel_distances.self_distance_matrix(members, window, penalty)``, unless ``distances`` -- that float32
           (m, m) matrix of the m members -- is given (no device is touched then);
        3. ``K = exp(-gamma * D ** pwr_dist)`` on the float32 matrix;
        4. ``SVC(kernel="precomputed", probability=True, C=C, random_state=random_state).fit(K, y[members])``;
        5. ``label_mapper = {i: classes_[i]}``, ``_X`` = the member rows.

        ``class_weight`` (``None``, ``"balanced"`` = n_members / (k * count), or a dict by label), ``tol`` and ``max_iter``
        (-1: libsvm's own cap, max(10 000 000, 100 * rows)) are the ``SVC``'s; the shipped reference models are
        ``C=1, class_weight="balanced", tol=1e-3``.

        ``solver="device"`` replaces step 4 by one batched launch of the engine's SMO solver (include/wdx.h:
        wdx_svm_solve_device states its rule; `_svm_fit` the host code around it): the same optimisation problems on the same
        ``K``, per pair ``c_pos = C * w_i``, ``c_neg = C * w_j``, stopped at the same gap ``tol`` -- so every pair's solution
        meets the KKT conditions to ``tol`` as libsvm's does, without being the same numbers.  ``probA`` / ``probB`` come from
        libsvm's ``sigmoid_train`` on five folds per pair which are THIS ENGINE'S OWN (scikit-learn's random generator cannot
        be reproduced; `_svm_fit` states the fold rule, seeded by ``random_state``, a non-negative integer): they differ from a
        libsvm fit's.  A pair of more than ``_lib.SVM_FIT_MAX_ROWS`` rows is ``NotImplementedError``.  The model carries
        ``fit_info_`` (per problem: pair, fold, rows, iterations, state), and a ``RuntimeWarning`` is raised when a problem's
        state is not 0.

        ``thresholds="cv"`` (``solver="device"`` only, ``ValueError`` otherwise) returns a DEPLOYABLE model, one with the
        per-class confidence thresholds every shipped model carries: the self-distance matrix, the kernel matrix and the solve
        stay on the device, the full data's problems and the ``cv`` outer folds' (`_svm_cv` states the folds) are one launch,
        and ``thresholds`` are those that reach ``target_accuracy`` (a whole number of per mille) on the out-of-fold
        probabilities -- the engine's own rule (include/wdx.h: wdx_accuracy_thresholds_device; the reference ships threshold tables
        but not the procedure behind them).  The model keeps ``cv_``: ``prob`` / ``pred`` / ``conf`` / ``fold`` as
        `cross_val_predict` returns them, the ``(1, k)`` table ``thresholds``, ``kept`` / ``hit`` / ``skipped`` and ``target``.
        On this route ``K`` comes from the engine's stated ``exp_rule`` (include/wdx.h: wdx_svm_kernel_device), not from
        ``numpy.exp``, and its argument is a float64 product: measured on a 16 384-row matrix (profiles/svm_cv.json), an entry lies
        at most 3 float32 ulps from step 3's and the decision values of the two fits differ by at most 5.8e-4, inside the
        stopping gap ``tol`` = 1e-3.  A class with
        fewer than ``cv`` members is ``ValueError``.

        ``ValueError`` before any device work: fewer than two classes among the members, more than 16 classes (the limit of
        the resident SVM tail), a ``y``, ``status`` or ``distances`` of the wrong shape, an unknown ``solver`` or
        ``class_weight``, a ``tol`` that is not positive, a bad ``max_iter``."""
        from sklearn.svm import SVC

        from . import _medoids

        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] < 1:
            raise ValueError(f"X must be (n, L) with L >= 1, got shape {X.shape}")
        X = np.ascontiguousarray(X, dtype=np.float64)
        n = X.shape[0]
        y = np.asarray(y)
        if y.shape != (n,):
            raise ValueError(f"y must hold one label per row: shape ({n},), not {y.shape}")
        if y.dtype.kind not in "iu":
            raise ValueError(f"y must have an integer dtype, not {y.dtype}")
        st = _medoids.host_status(n, status)
        member = np.isfinite(X).all(axis=1)
        if st is not None:
            member &= st == 0
        Xm, ym = np.ascontiguousarray(X[member]), y[member]
        m = int(member.sum())
        if distances is not None:
            distances = np.asarray(distances)
            if distances.shape != (m, m):
                raise ValueError(f"distances must be the ({m}, {m}) matrix of the {m} members, not {distances.shape}")
        classes = np.unique(ym)
        if classes.size < 2:
            raise ValueError(f"fit needs at least two classes among the members, found {classes.size}")
        if classes.size > _lib.SVM_MAX_CLASSES:
            raise ValueError(f"{classes.size} classes: the resident SVM tail serves at most {_lib.SVM_MAX_CLASSES}")
        want_cv = isinstance(thresholds, str)
        if want_cv and thresholds != "cv":
            raise ValueError(f'thresholds must be None, one value per class or "cv", not {thresholds!r}')
        if not want_cv and thresholds is not None and np.asarray(thresholds).shape != (classes.size,):
            raise ValueError(f"thresholds must hold one value per class: shape ({classes.size},), not {np.asarray(thresholds).shape}")
        if solver not in ("libsvm", "device"):
            raise ValueError(f'solver must be "libsvm" or "device", not {solver!r}')
        if want_cv and solver != "device":
            raise ValueError('thresholds="cv" needs solver="device"')
        if solver == "device":
            from . import _svm_fit

            for name, v in (("tol", tol), ("C", C)):
                if not (np.isscalar(v) and np.isreal(v) and np.isfinite(v) and v > 0):
                    raise ValueError(f"{name} must be positive and finite, not {v!r}")
            y_idx = np.searchsorted(classes, ym)
            weights = _svm_fit.class_weights(class_weight, classes, y_idx)
            _svm_fit.effective_max_iter(max_iter, 0)
            if not isinstance(random_state, (int, np.integer)) or random_state < 0:
                raise ValueError(f'solver="device" needs a non-negative integer random_state, not {random_state!r}')
            counts = np.bincount(y_idx)
            if np.sort(counts)[-2:].sum() > _lib.SVM_FIT_MAX_ROWS:
                raise NotImplementedError(f"the two largest classes hold {int(np.sort(counts)[-2:].sum())} rows, more than "
                                          f"WDX_SVM_FIT_MAX_ROWS = {_lib.SVM_FIT_MAX_ROWS}: subsample them, or fit with solver='libsvm'")
        elif not (class_weight is None or class_weight == "balanced" or isinstance(class_weight, dict)):
            raise ValueError(f'class_weight must be None, "balanced" or a dict, not {class_weight!r}')
        if want_cv:
            from . import _svm_cv, _thresholds

            _svm_cv.check_cv(cv, counts)
            target = _thresholds.targets_per_mille([target_accuracy])
            res = _svm_cv_on_device(Xm, y_idx, classes, window, penalty, gamma, pwr_dist, C, class_weight, tol, max_iter, random_state, cv,
                                    True, device, distances=distances, targets=[target_accuracy])
            n_support, support, dual, rho, probA, probB = res["full"]
            model = cls(Xm, n_support, support, dual, rho, probA, probB, {i: int(c) for i, c in enumerate(classes)}, res["thresholds"][0],
                        window, penalty, gamma=gamma, pwr_dist=pwr_dist, block_size=block_size, device=device)
            info = res["fit_info"]
            full = info["part"] == cv
            model.fit_info_ = {"pairs": info["pairs"], **{key: info[key][full] for key in ("pair", "fold", "rows", "n_iter", "state")}}
            model.cv_ = {key: res[key] for key in ("prob", "pred", "conf", "fold", "thresholds", "kept", "hit", "skipped")}
            model.cv_["target"] = int(target[0]) / 1000
            model.cv_["fit_info"] = info
            if (info["state"] != 0).any():
                import warnings

                warnings.warn(f"DTW_SVM.fit: {int((info['state'] != 0).sum())} of {len(info['state'])} problems did not converge "
                              f"(states {sorted(set(int(s) for s in info['state']))}: 1 = iteration cap, 2 = stopped)", RuntimeWarning)
            model.n_dropped_ = n - m
            return model
        if distances is None:
            from .parallel_distances import self_distance_matrix

            D = self_distance_matrix(Xm, window=window, penalty=penalty)
        else:
            D = np.ascontiguousarray(distances, dtype=np.float32)
        K = np.exp(-gamma * np.power(D, pwr_dist))   # the reference's pdist_kernel on the float32 matrix
        if solver == "device":
            import warnings

            n_support, support, dual, rho, probA, probB, info = _svm_fit.fit_arrays(
                K, y_idx, classes.size, C * weights, tol, max_iter, random_state,
                lambda K_, batch, eps, cap: _svm_fit.solve_host(K_, batch, eps, cap, device=device))
            model = cls(Xm, n_support, support, dual, rho, probA, probB, {i: int(c) for i, c in enumerate(classes)}, thresholds, window,
                        penalty, gamma=gamma, pwr_dist=pwr_dist, block_size=block_size, device=device)
            model.fit_info_ = info
            if (info["state"] != 0).any():
                warnings.warn(f"DTW_SVM.fit: {int((info['state'] != 0).sum())} of {len(info['state'])} problems did not converge "
                              f"(states {sorted(set(int(s) for s in info['state']))}: 1 = iteration cap, 2 = stopped)", RuntimeWarning)
        else:
            svc = SVC(kernel="precomputed", probability=True, C=C, random_state=random_state, class_weight=class_weight, tol=tol,
                      max_iter=max_iter).fit(K, ym)
            model = cls.from_sklearn(svc, Xm, {i: int(c) for i, c in enumerate(svc.classes_)}, thresholds, window, penalty, gamma=gamma,
                                     pwr_dist=pwr_dist, block_size=block_size, device=device)
        model.n_dropped_ = n - m
        return model

    @classmethod
    def cross_val_predict(cls, X, y, window, penalty, gamma=1.0, pwr_dist=1, C=1.0, class_weight=None, tol=1e-3, max_iter=-1,
                          random_state=0, cv=5, status=None, device: Optional[int] = None):
        """``(y_prob float64 (m, k), y_pred int64 (m,), conf float64 (m,), fold int32 (m,))`` on the m member rows (as `fit`
        finds them): every row's probabilities from the model of the fold that holds it out -- what a threshold is calibrated
        on.  The self-distance matrix, the kernel matrix (``exp_rule``: see `fit`) and the one batched solve of all ``cv`` folds
        stay on the device; over the bus come the solve's results for `_svm_fit.sigmoid_train`, and these four arrays.
        ``y_pred`` holds labels (columns of ``y_prob``: the sorted labels), -1 where a problem of the row's fold stopped (NaN
        probabilities).  The folds are the engine's own (`_svm_cv`), seeded by ``random_state``.  A class with fewer than
        ``cv`` members (2 <= cv <= 10) is ``ValueError`` before any device work."""
        from . import _medoids, _svm_cv

        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] < 1:
            raise ValueError(f"X must be (n, L) with L >= 1, got shape {X.shape}")
        X = np.ascontiguousarray(X, dtype=np.float64)
        n = X.shape[0]
        y = np.asarray(y)
        if y.shape != (n,) or y.dtype.kind not in "iu":
            raise ValueError(f"y must hold one integer label per row: shape ({n},)")
        st = _medoids.host_status(n, status)
        member = np.isfinite(X).all(axis=1)
        if st is not None:
            member &= st == 0
        Xm, ym = np.ascontiguousarray(X[member]), y[member]
        classes = np.unique(ym)
        if not 2 <= classes.size <= _lib.SVM_MAX_CLASSES:
            raise ValueError(f"{classes.size} classes among the members (2..{_lib.SVM_MAX_CLASSES})")
        y_idx = np.searchsorted(classes, ym)
        _svm_cv.check_cv(cv, np.bincount(y_idx))
        res = _svm_cv_on_device(Xm, y_idx, classes, window, penalty, gamma, pwr_dist, C, class_weight, tol, max_iter, random_state, cv, False,
                                device)
        return res["prob"], res["pred"], res["conf"], res["fold"]

    @property
    def num_bcs(self):
        return self.n_classes

    def to_c(self) -> "_lib.SvmModelC":
        """wdx_svm_model view of the host arrays (valid while ``self`` is alive)."""
        return _lib.SvmModelC(
            self.n_classes, int(self._support.size), int(self._X.shape[0]), self.pwr_dist, self.gamma,
            self._n_support.ctypes.data, self._support.ctypes.data, self._dual_coef.ctypes.data,
            self._rho.ctypes.data, self._probA.ctypes.data, self._probB.ctypes.data, self._label_arr.ctypes.data,
            None if self.thresholds is None else self.thresholds.ctypes.data,
        )

    def _column_error(self) -> str:
        return f"X must have the same number of columns as the training data  ({self._X.shape[1]})."

    def predict(self, X: np.ndarray, nproc: int = -1, block_size: Optional[int] = None, pbar: bool = False,
                pbar_kwargs: dict = {}, return_df: bool = False) -> Union[Tuple[np.ndarray, np.ndarray], "object"]:
        """(y_pred, y_prob) or the predictions DataFrame -- dtw_svm.py:54-98.  ``nproc`` / ``block_size``
        keep the reference's validation (block_size required when nproc != 1) but nothing is forked."""
        ctx, X, y_prob, y_pred, conf = self._predict_inputs(X, nproc, block_size, self.n_classes)
        _lib.check(_lib.load().wdx_dtw_svm_predict(ctx.handle, _lib.ptr(X), X.shape[0], _lib.ptr(y_prob), _lib.ptr(y_pred),
                                                   _lib.ptr(conf)))
        y_pred = y_pred.astype(np.int64)
        if return_df:
            return predictions_to_df(y_pred, y_prob, conf, self.label_mapper)
        return y_pred, y_prob


def _sklearn_mlp_parts(est):
    """(scaler steps [(mean_ or None, scale_ or None)], MLPClassifier) of ``model.model``: zero or more
    StandardScaler steps and one MLPClassifier (BaseDTWModel types it Union[Pipeline, SVC]).  Anything else is refused."""
    from sklearn.neural_network import MLPClassifier
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler

    steps = [s for _, s in est.steps] if isinstance(est, Pipeline) else [est]
    steps = [s for s in steps if s is not None and s != "passthrough"]
    if not steps or not isinstance(steps[-1], MLPClassifier):
        raise ValueError("expected an MLPClassifier, optionally behind StandardScaler steps")
    scalers = []
    for s in steps[:-1]:
        # (subclasses such as warpdemux's WeightedStandardScaler only change fit: transform is StandardScaler's)
        if not isinstance(s, StandardScaler) or type(s).transform is not StandardScaler.transform:
            raise ValueError(f"unsupported pipeline step {type(s).__name__}: only StandardScaler steps may precede the MLP")
        mean = getattr(s, "mean_", None) if s.with_mean else None
        scale = getattr(s, "scale_", None) if s.with_std else None
        scalers.append((mean, scale))
    return scalers, steps[-1]


class DTW_MLP(_ResidentDTWModel):
    """``warpdemux.models.dtw_mlp.DTW_MLP`` with the classifier tail resident on one GPU context: DTW distances to
    ``_X`` -> StandardScaler steps -> ``MLPClassifier.predict_proba`` -> ``process_probs``, the (n, len(_X)) distance
    matrix never leaving HBM.  The working dtype is scikit-learn's: ``result_type(float32, coefs_[0].dtype)``.  The MLP
    slot of the context is separate from the SVM's, so a resident SVM stays as it is."""

    _owner_attr = "_mlp_owner"

    def __init__(self, _X: np.ndarray, coefs, intercepts, activation: str, label_mapper: Dict[int, int],
                 thresholds: Optional[np.ndarray], window: int, penalty: float, scalers=(), n_classes: Optional[int] = None,
                 noise_class: bool = False, block_size: Optional[int] = None, out_activation: Optional[str] = None,
                 device: Optional[int] = None):
        self._init_common(_X, window, penalty, block_size, label_mapper, thresholds, device)
        self.dtype = np.result_type(np.float32, np.asarray(coefs[0]).dtype)
        if self.dtype not in (np.float32, np.float64):
            raise ValueError(f"unsupported MLP dtype {self.dtype}")
        self._coefs = [np.ascontiguousarray(c, dtype=self.dtype) for c in coefs]
        self._intercepts = [np.ascontiguousarray(b, dtype=self.dtype) for b in intercepts]
        if activation not in _lib.MLP_ACT:
            raise ValueError(f"unknown activation {activation!r}")
        self.activation = activation
        n_out = self._coefs[-1].shape[1]
        self.out_activation = out_activation or ("logistic" if n_out == 1 else "softmax")
        if (self.out_activation == "logistic") != (n_out == 1) or self.out_activation not in ("logistic", "softmax"):
            raise ValueError(f"unsupported output layer: {self.out_activation} over {n_out} units")
        self._scalers = [(None if m is None else np.ascontiguousarray(m, dtype=np.float64),
                          None if s is None else np.ascontiguousarray(s, dtype=np.float64)) for m, s in scalers]
        self.n_outputs = n_out
        self.k = 2 if n_out == 1 else n_out
        self.n_classes = n_classes
        self.noise_class = noise_class
        self._label_arr = np.array([self.label_mapper[i] for i in range(self.k)], dtype=np.int32)

    @classmethod
    def from_reference(cls, model, device: Optional[int] = None) -> "DTW_MLP":
        """From a reference ``DTW_MLP`` instance: reads ``model.model`` (an MLPClassifier, or a Pipeline of StandardScaler
        steps and one), ``_X``, ``window``, ``penalty``, ``block_size``, ``label_mapper``, ``thresholds``."""
        scalers, mlp = _sklearn_mlp_parts(model.model)
        return cls(
            _X=model._X, coefs=mlp.coefs_, intercepts=mlp.intercepts_, activation=mlp.activation,
            out_activation=mlp.out_activation_, scalers=scalers, label_mapper=model.label_mapper,
            thresholds=model.thresholds, window=model.window, penalty=model.penalty, block_size=model.block_size,
            n_classes=getattr(model, "n_classes", None), noise_class=getattr(model, "noise_class", False), device=device,
        )

    @classmethod
    def fit(cls, X, y, window, penalty, refs=None, hidden_layer_sizes=(100,), activation="relu", alpha=1e-4, batch_size="auto",
            learning_rate_init=1e-3, max_iter=200, tol=1e-4, n_iter_no_change=10, shuffle=True, random_state=0, beta_1=0.9,
            beta_2=0.999, epsilon=1e-8, scale=True, thresholds=None, status=None, distances=None, solver="device",
            block_size: Optional[int] = None, device: Optional[int] = None) -> "DTW_MLP":
        """Train a model on labelled fingerprints ``X`` (n, L), ``y`` (n,) integer barcode labels: the reference's DTW_MLP -- DTW
        distances to a reference set, a ``StandardScaler``, an ``MLPClassifier(solver="adam")`` -- fitted in float32.

        1. members only: a row with a sample that is not finite, or whose ``status`` (optional, one integer per row) is not 0,
           is dropped; their number is ``n_dropped_`` of the returned model;
        2. ``_X`` = ``refs`` (nY, L), for example the barycenters of `parallel_distances.label_barycenters`; ``None``: the
           members themselves;
        3. ``D = distance_matrix_to(members, _X, window, penalty)``, unless ``distances`` -- that float32 (m, nY) matrix of the
           m members -- is given;
        4. with ``scale``: ``mean_`` / ``scale_`` of a host ``StandardScaler().fit(D)``;
        5. ``solver="device"``: the initial weights and every epoch's row order are drawn from ``RandomState(random_state)``
           exactly as scikit-learn draws them (`_mlp_fit.schedule`; a non-negative integer seed), and the engine's trainer
           (include/wdx.h: wdx_mlp_fit_device states its rule) follows scikit-learn's float32 trajectory with rounding as the only
           difference.  ``solver="sklearn"``: the ``StandardScaler`` + ``MLPClassifier`` pipeline itself on the host matrix;
        6. ``label_mapper = {i: classes_[i]}``.

        ``batch_size="auto"`` is scikit-learn's ``min(200, m)``.  The model carries ``loss_curve_`` and ``n_iter_``; a
        ``RuntimeWarning`` is raised when ``max_iter`` ends the fit with ``tol > 0``.  ``ValueError`` before any device work:
        bad shapes, fewer than two classes among the members, more than 16 classes, an unknown ``solver`` or ``activation``, a
        ``tol`` or ``learning_rate_init`` that is not positive; a limit of the trainer exceeded is ``NotImplementedError``
        (`_lib.MLP_FIT_MAX_BATCH`, the tail's layers and widths).  A distance or scaled input that is not finite is
        ``ValueError`` once the device has found it."""
        import warnings

        from . import _medoids, _mlp_fit

        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] < 1:
            raise ValueError(f"X must be (n, L) with L >= 1, got shape {X.shape}")
        X = np.ascontiguousarray(X, dtype=np.float64)
        n = X.shape[0]
        y = np.asarray(y)
        if y.shape != (n,):
            raise ValueError(f"y must hold one label per row: shape ({n},), not {y.shape}")
        if y.dtype.kind not in "iu":
            raise ValueError(f"y must have an integer dtype, not {y.dtype}")
        st = _medoids.host_status(n, status)
        member = np.isfinite(X).all(axis=1)
        if st is not None:
            member &= st == 0
        Xm, ym = np.ascontiguousarray(X[member]), y[member]
        m = int(member.sum())
        if refs is None:
            R = Xm
        else:
            R = np.asarray(refs)
            if R.ndim != 2 or R.shape[1] != X.shape[1] or R.shape[0] < 1:
                raise ValueError(f"refs must be (nY, {X.shape[1]}) with nY >= 1, got shape {R.shape}")
            R = np.ascontiguousarray(R, dtype=np.float64)
        nY = R.shape[0]
        if distances is not None:
            distances = np.asarray(distances)
            if distances.shape != (m, nY):
                raise ValueError(f"distances must be the ({m}, {nY}) matrix of the {m} members, not {distances.shape}")
        classes = np.unique(ym)
        if classes.size < 2:
            raise ValueError(f"fit needs at least two classes among the members, found {classes.size}")
        if classes.size > _lib.MLP_FIT_MAX_CLASSES:
            raise ValueError(f"{classes.size} classes: the resident MLP tail serves at most {_lib.MLP_FIT_MAX_CLASSES}")
        if thresholds is not None and np.asarray(thresholds).shape != (classes.size,):
            raise ValueError(f"thresholds must hold one value per class: shape ({classes.size},), not {np.asarray(thresholds).shape}")
        if solver not in ("device", "sklearn"):
            raise ValueError(f'solver must be "device" or "sklearn", not {solver!r}')
        if activation not in _mlp_fit.ACTIVATIONS:
            raise ValueError(f"unknown activation {activation!r}: one of {_mlp_fit.ACTIVATIONS}")
        for name, v in (("tol", tol), ("learning_rate_init", learning_rate_init)):
            if not (np.isscalar(v) and np.isreal(v) and np.isfinite(v) and v > 0):
                raise ValueError(f"{name} must be positive and finite, not {v!r}")
        if batch_size == "auto":
            bs = min(200, m)
        elif isinstance(batch_size, (int, np.integer)) and batch_size >= 1:
            bs = int(batch_size)
        else:
            raise ValueError(f'batch_size must be "auto" or a positive integer, not {batch_size!r}')
        y_idx = np.searchsorted(classes, ym).astype(np.int32)
        mapper = {i: int(c) for i, c in enumerate(classes)}
        if solver == "device":
            sizes = _mlp_fit.layer_sizes(nY, hidden_layer_sizes, classes.size)
            p = _mlp_fit.params_c(sizes, activation, classes.size, bs, max_iter, n_iter_no_change, learning_rate_init, alpha, beta_1,
                                  beta_2, epsilon, tol)
            _mlp_fit.check_seed(random_state)
        if distances is None:
            from .parallel_distances import distance_matrix_to

            D = distance_matrix_to(Xm, R, window=window, penalty=penalty, n_jobs=1)
        D = np.ascontiguousarray(D if distances is None else distances, dtype=np.float32)
        if solver == "sklearn":
            from sklearn.exceptions import ConvergenceWarning
            from sklearn.neural_network import MLPClassifier
            from sklearn.pipeline import make_pipeline
            from sklearn.preprocessing import StandardScaler

            mlp = MLPClassifier(hidden_layer_sizes=hidden_layer_sizes, activation=activation, solver="adam", alpha=alpha, batch_size=bs,
                                learning_rate_init=learning_rate_init, max_iter=max_iter, tol=tol, n_iter_no_change=n_iter_no_change,
                                shuffle=shuffle, random_state=random_state, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon)
            est = make_pipeline(StandardScaler(), mlp) if scale else mlp
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", ConvergenceWarning)
                est.fit(D, y_idx)
            scalers, mlp = _sklearn_mlp_parts(est)
            model = cls(R, mlp.coefs_, mlp.intercepts_, activation, mapper, thresholds, window, penalty, scalers=scalers,
                        n_classes=classes.size, block_size=block_size, out_activation=mlp.out_activation_, device=device)
            model.loss_curve_, model.n_iter_ = np.asarray(mlp.loss_curve_, dtype=np.float64), int(mlp.n_iter_)
            hit_cap = model.n_iter_ == max_iter
        else:
            mean = scl = None
            if scale:
                from sklearn.preprocessing import StandardScaler

                if not np.isfinite(D).all():
                    raise ValueError("DTW_MLP.fit: a distance is not finite")
                sc = StandardScaler().fit(D)
                mean, scl = sc.mean_, sc.scale_
            W0, B0, order = _mlp_fit.schedule(sizes, activation, random_state, m, int(max_iter), shuffle)
            W0, B0, mean, scl, order = _mlp_fit.check_arrays(sizes, m, W0, B0, mean, scl, order, int(max_iter))
            res = _mlp_fit.fit_host(D, y_idx, p, W0, B0, mean, scl, order, device=device)
            if res.state in ("nonfinite_input", "nonfinite_loss"):
                raise ValueError("DTW_MLP.fit: " + ("a scaled distance is not finite" if res.state == "nonfinite_input" else
                                                    f"the loss of epoch {res.n_iter} is not finite"))
            model = cls(R, res.coefs, res.intercepts, activation, mapper, thresholds, window, penalty,
                        scalers=[(mean, scl)] if scale else (), n_classes=classes.size, block_size=block_size, device=device)
            model.loss_curve_, model.n_iter_ = res.loss_curve, res.n_iter
            hit_cap = res.state == "max_epochs"
        if hit_cap and tol > 0:
            warnings.warn(f"DTW_MLP.fit: max_iter = {max_iter} reached and the optimisation has not converged yet", RuntimeWarning)
        model.n_dropped_ = n - m
        return model

    def num_bcs(self) -> int:
        """dtw_mlp.py:95-100"""
        if self.n_classes is not None:
            return self.n_classes
        if self.label_mapper is not None:
            return len(self.label_mapper) - self.noise_class
        raise ValueError("No number of barcodes available.")

    def to_c(self) -> "_lib.MlpModelC":
        """wdx_mlp_model view of the host arrays (valid while ``self`` is alive)."""
        m = _lib.MlpModelC()
        nl = len(self._coefs)
        m.n_layers = nl
        m.dtype_bytes = self.dtype.itemsize
        m.hidden_activation = _lib.MLP_ACT[self.activation]
        m.n_classes = self.k
        m.n_scalers = len(self._scalers)
        if nl > _lib.MLP_MAX_LAYERS or len(self._scalers) > _lib.MLP_MAX_SCALERS:
            return m   # (the counts alone: the library refuses the model before it reads an array)
        m.sizes[0] = self._coefs[0].shape[0]
        for i, (c, b) in enumerate(zip(self._coefs, self._intercepts)):
            m.sizes[i + 1] = c.shape[1]
            m.coefs[i] = c.ctypes.data
            m.intercepts[i] = b.ctypes.data
        for i, (mean, scale) in enumerate(self._scalers):
            m.scaler_mean[i] = None if mean is None else mean.ctypes.data
            m.scaler_scale[i] = None if scale is None else scale.ctypes.data
        m.label_map = self._label_arr.ctypes.data
        m.thresholds = None if self.thresholds is None else self.thresholds.ctypes.data
        return m

    def _column_error(self) -> str:
        return f"X must have the same shape in axis 1 as the consensus sequences  ({self._X.shape})."

    def _nonfinite_message(self, X) -> str:
        """scikit-learn's first line for the distances of X (error path only: the distances are recomputed to the host)."""
        from .parallel_distances import distance_matrix_to

        D = distance_matrix_to(X, self._X, window=self.window, penalty=self.penalty, n_jobs=1)
        inf_msg = "Input X contains infinity or a value too large for dtype('float32')."
        for mean, scale in self._scalers:     # StandardScaler.transform: allow-nan validation
            if np.isinf(D).any():
                return inf_msg
            with np.errstate(all="ignore"):
                if mean is not None:
                    D -= mean
                if scale is not None:
                    D /= scale
        if np.isnan(D).any():
            return "Input X contains NaN."
        return inf_msg

    def predict(self, X: np.ndarray, nproc: int = -1, block_size: Optional[int] = None, pbar: bool = False,
                pbar_kwargs: dict = {}, return_df: bool = False) -> Union[Tuple[np.ndarray, np.ndarray], "object"]:
        """(y_pred, y_prob) or the predictions DataFrame -- dtw_mlp.py:44-93.  ``nproc`` / ``block_size`` keep the
        reference's validation (distance_matrix_to wants block_size when nproc != 1) but nothing is forked."""
        ctx, X, y_prob, y_pred, conf = self._predict_inputs(X, nproc, block_size, self.k)
        bad = C.c_int64(0)
        _lib.check(_lib.load().wdx_dtw_mlp_predict(ctx.handle, _lib.ptr(X), X.shape[0], _lib.ptr(y_prob), _lib.ptr(y_pred),
                                                   _lib.ptr(conf), C.byref(bad)))
        if bad.value:
            raise ValueError(self._nonfinite_message(X))
        y_prob = y_prob.astype(self.dtype)      # exact: float32 models return float32 values widened
        y_pred = y_pred.astype(np.int64)
        if return_df:
            if self.label_mapper is None:
                raise ValueError("Label mapper is not set.")
            return predictions_to_df(y_pred, y_prob, conf.astype(self.dtype), self.label_mapper)
        return y_pred, y_prob


_NAN_TRUE = {"AsIs": 0, "AsFalse": 0, "AsTrue": 1}   # features_info.float_features[*].nan_value_treatment


class Fpt_Boost:
    """``warpdemux.models.fpt_boost.Fpt_Boost`` with the classifier resident on one GPU context (wdx_boost.hip; DESIGN.md
    4.8): an ensemble of oblivious trees over the float64 fingerprint (rounded to float32 once) -> ``scale * sum + bias`` ->
    softmax / sigmoid -> ``process_probs``.  No DTW and no reference set.  The contract is the NumPy restatement in
    tests/helpers/boost_ref.py; parity with CatBoost's own evaluation is not pinned.

    ``trees``: a sequence of ``(features int[depth], borders float32[depth], nan_true bool[depth], leaves float64
    (2**depth, dim))``; split ``i`` of a tree sets bit ``i`` of the leaf index, ``leaves[leaf, c]`` is class ``c``'s value.
    The boost slot of the context is separate from the SVM's and the MLP's."""

    _owner_attr = "_boost_owner"

    def __init__(self, trees, n_features: int, scale: float, bias, label_mapper: Optional[Dict[int, int]],
                 thresholds: Optional[np.ndarray] = None, n_classes: Optional[int] = None, noise_class: bool = False,
                 device: Optional[int] = None):
        bias = np.atleast_1d(np.asarray(bias, dtype=np.float64))
        self.dim = int(bias.size)
        self.k = 2 if self.dim == 1 else self.dim
        self.n_features = int(n_features)
        self._depth = np.array([len(t[0]) for t in trees], dtype=np.int32)
        cat = lambda i, dt: np.ascontiguousarray(   # noqa: E731
            np.concatenate([np.asarray(t[i], dtype=dt).ravel() for t in trees]) if len(trees) else np.zeros(0, dt), dtype=dt)
        self._split_feature = cat(0, np.int32)
        self._split_border = cat(1, np.float32)
        self._split_nan_true = cat(2, np.uint8)
        for t, d in zip(trees, self._depth):
            if np.asarray(t[3]).size != (1 << int(d)) * self.dim or not (len(t[1]) == len(t[2]) == d):
                raise ValueError(f"a tree of depth {d} needs {d} borders / NaN rules and {(1 << int(d)) * self.dim} leaf values")
        self._leaf_values = cat(3, np.float64)
        self.scale = float(scale)
        self._bias = np.ascontiguousarray(bias)
        self.label_mapper = None if label_mapper is None else dict(label_mapper)
        self.thresholds = None if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64)
        self.n_classes, self.noise_class = n_classes, noise_class
        self._device = device
        self._check_limits()
        if self.label_mapper:
            self._label_arr = np.array([self.label_mapper[i] for i in range(self.k)], dtype=np.int32)
        if self.thresholds is not None and self.thresholds.size != self.k:
            raise ValueError(f"{self.thresholds.size} thresholds for {self.k} classes")

    def _check_limits(self):
        """The kernel's limits (include/wdx.h), refused here as the library would."""
        if len(self._depth) < 1:   # (an untrained model: predict says so)
            return
        if not 1 <= self.n_features <= _lib.BOOST_MAX_FEATURES:
            raise NotImplementedError(f"{self.n_features} features (1..{_lib.BOOST_MAX_FEATURES} supported)")
        if self._depth.max() > _lib.BOOST_MAX_DEPTH:
            raise NotImplementedError(f"tree depth {int(self._depth.max())} (0..{_lib.BOOST_MAX_DEPTH} supported)")
        if self.dim > _lib.BOOST_MAX_DIM:
            raise NotImplementedError(f"{self.dim} classes (2..{_lib.BOOST_MAX_DIM} supported)")
        if self._split_feature.size and not (0 <= self._split_feature.min() and self._split_feature.max() < self.n_features):
            raise ValueError("a split tests a feature the model does not have")

    # -- loaders: the two conventions of CatBoost's JSON model format are fixed HERE (and in the tests' restatement) ------
    @classmethod
    def from_json(cls, path_or_dict, label_mapper, thresholds=None, n_classes=None, noise_class=False,
                  device: Optional[int] = None) -> "Fpt_Boost":
        """From a CatBoost JSON model (``save_model(..., format="json")``), a path or the parsed dict.  Read:
        ``oblivious_trees[*].splits[*].{float_feature_index, border, split_type}`` (``splits[i]`` sets bit ``i`` of the leaf
        index), ``oblivious_trees[*].leaf_values`` (leaf-major, class fastest: ``leaf_values[leaf * dim + c]``),
        ``features_info.float_features[*].nan_value_treatment``, ``scale_and_bias`` and the class count
        (``model_info.class_params``, else the length of the bias)."""
        if isinstance(path_or_dict, dict):
            js = path_or_dict
        else:
            import json

            with open(path_or_dict) as fh:
                js = json.load(fh)
        if "oblivious_trees" not in js:
            if "trees" in js:
                raise NotImplementedError("non-symmetric trees are not supported (oblivious trees only)")
            raise ValueError("not a CatBoost JSON model: no 'oblivious_trees'")
        info = js.get("features_info", {})
        for key, what in (("categorical_features", "categorical"), ("text_features", "text"),
                          ("embedding_features", "embedding"), ("ctrs", "categorical (ctr)")):
            if info.get(key):
                raise NotImplementedError(f"{what} features are not supported (float features only)")
        ff = info.get("float_features") or []
        if not ff:
            raise ValueError("no float features in features_info")
        # a split names a float feature by its position in float_features; the column of X is its flat index
        column = [int(f.get("flat_feature_index", f.get("feature_index", i))) for i, f in enumerate(ff)]
        nan_true = []
        for f in ff:
            tr = f.get("nan_value_treatment", "AsIs")
            if tr not in _NAN_TRUE:
                raise NotImplementedError(f"nan_value_treatment {tr!r}")
            nan_true.append(_NAN_TRUE[tr])
        n_features = max(column) + 1
        sb = js.get("scale_and_bias", [1.0, [0.0]])
        scale = float(sb[0])
        bias = np.atleast_1d(np.asarray(sb[1], dtype=np.float64))
        trees_js = js["oblivious_trees"]
        if not trees_js:
            raise ValueError("a boost model needs at least one tree")
        # values per leaf: the first tree's table over its leaf count
        d0 = len(trees_js[0].get("splits") or [])
        dim, rem = divmod(len(trees_js[0]["leaf_values"]), 1 << min(d0, 40))
        if rem or dim < 1:
            raise ValueError("leaf_values is not a multiple of 2**depth")
        if bias.size == 1 and dim > 1:
            bias = np.repeat(bias, dim)
        if bias.size != dim:
            raise ValueError(f"{bias.size} bias values for {dim} values per leaf")
        cp = (js.get("model_info") or {}).get("class_params") or {}
        names = cp.get("class_names") or cp.get("class_to_label") or []
        k = len(names) if names else (2 if dim == 1 else dim)
        if k != (2 if dim == 1 else dim):
            raise ValueError(f"{k} classes for {dim} values per leaf")
        if dim > _lib.BOOST_MAX_DIM:
            raise NotImplementedError(f"{dim} classes (2..{_lib.BOOST_MAX_DIM} supported)")
        trees = []
        for t in trees_js:
            sp = t.get("splits") or []
            if len(sp) > _lib.BOOST_MAX_DEPTH:
                raise NotImplementedError(f"tree depth {len(sp)} (0..{_lib.BOOST_MAX_DEPTH} supported)")
            for s_ in sp:
                if s_.get("split_type", "FloatFeature") != "FloatFeature":
                    raise NotImplementedError(f"split type {s_.get('split_type')!r} is not supported (FloatFeature only)")
            idx = [int(s_["float_feature_index"]) for s_ in sp]
            if any(i < 0 or i >= len(ff) for i in idx):
                raise ValueError("a split names a float feature the model does not have")
            lv = np.asarray(t["leaf_values"], dtype=np.float64)
            if lv.size != (1 << len(sp)) * dim:
                raise ValueError(f"a tree of depth {len(sp)} has {lv.size} leaf values, expected {(1 << len(sp)) * dim}")
            trees.append(([column[i] for i in idx], [np.float32(s_["border"]) for s_ in sp], [nan_true[i] for i in idx],
                          lv.reshape(1 << len(sp), dim)))
        return cls(trees, n_features, scale, bias, label_mapper, thresholds, n_classes=n_classes, noise_class=noise_class,
                   device=device)

    @classmethod
    def from_reference(cls, model, device: Optional[int] = None) -> "Fpt_Boost":
        """From a reference ``Fpt_Boost`` instance: ``model.model.save_model(tmp, format="json")`` in a temporary
        directory, then ``from_json``.  (``model.model`` is only asked to write itself; nothing here imports its library.)"""
        import os
        import tempfile

        if getattr(model, "model", None) is None:
            msg = "Model not trained."
            logging.error(msg)
            raise ValueError(msg)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "model.json")
            model.model.save_model(path, format="json")
            return cls.from_json(path, model.label_mapper, model.thresholds, n_classes=getattr(model, "n_classes", None),
                                 noise_class=getattr(model, "noise_class", False), device=device)

    @classmethod
    def fit(cls, X, y, n_trees=1000, depth=6, learning_rate=0.1, l2_leaf_reg=3.0, border_count=128, label_mapper=None,
            thresholds=None, status=None, device: Optional[int] = None) -> "Fpt_Boost":
        """Train a model on labelled fingerprints ``X`` (n, F), ``y`` (n,) integer barcode labels, on the device: gradient
        boosting of oblivious trees on the raw fingerprint, MultiClass with one value per class and leaf (also for two classes).
        The rule is this engine's own (include/wdx.h: wdx_boost_fit_device states it bit for bit, tests/helpers/boost_fit_rule.py
        restates it in NumPy; `_boost_fit` holds the borders rule); parity with CatBoost's trainer is not a goal -- no ordered
        boosting, random strength or bootstrap, no sample or class weights, no early stopping.

        1. members only: a row whose ``status`` (optional, one integer per row) is not 0 is dropped; their number is
           ``n_dropped_`` of the returned model.  A NaN feature value is data: it falls into the feature's lowest bin;
        2. ``borders = _boost_fit.borders(members, border_count)`` on the host;
        3. ``n_trees`` trees of ``depth`` levels from zero scores through ``wdx_boost_fit``;
        4. ``label_mapper`` defaults to ``{i: classes[i]}`` of the sorted labels; a given one must map 0 .. k-1 onto them.

        The returned model is resident-ready (``scale = 1``, ``bias = 0``, ``nan_true = 0``) and carries ``train_scores`` (m, k):
        the trainer's final scores of the members, which are bit for bit what ``predict_raw(members)[0]`` returns, and
        ``borders_``.  ``ValueError`` / ``NotImplementedError`` before any device work for what `_boost_fit.params_c` names."""
        from . import _boost_fit, _medoids

        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] < 1:
            raise ValueError(f"X must be (n, F) with F >= 1, got shape {X.shape}")
        X = np.ascontiguousarray(X, dtype=np.float64)
        n = X.shape[0]
        y = np.asarray(y)
        if y.shape != (n,):
            raise ValueError(f"y must hold one label per row: shape ({n},), not {y.shape}")
        if y.dtype.kind not in "iu":
            raise ValueError(f"y must have an integer dtype, not {y.dtype}")
        st = _medoids.host_status(n, status)
        member = np.ones(n, dtype=bool) if st is None else st == 0
        Xm, ym = np.ascontiguousarray(X[member]), y[member]
        m = int(member.sum())
        classes = np.unique(ym)
        k = int(classes.size)
        if label_mapper is None:
            label_mapper = {i: int(c) for i, c in enumerate(classes)}
            y_idx = np.searchsorted(classes, ym)
        else:
            label_mapper = {int(i): int(c) for i, c in dict(label_mapper).items()}
            if sorted(label_mapper) != list(range(k)) or sorted(label_mapper.values()) != [int(c) for c in classes]:
                raise ValueError(f"label_mapper must map 0 .. {k - 1} onto the {k} labels among the members")
            inverse = {c: i for i, c in label_mapper.items()}
            y_idx = np.array([inverse[int(c)] for c in ym], dtype=np.int64)
        if thresholds is not None and np.asarray(thresholds).shape != (k,):
            raise ValueError(f"thresholds must hold one value per class: shape ({k},), not {np.asarray(thresholds).shape}")
        p = _boost_fit.params_c(X.shape[1], k, n_trees, depth, border_count, learning_rate, l2_leaf_reg)
        if m > _lib.BOOST_FIT_MAX_ROWS:
            raise NotImplementedError(f"{m} rows (1..{_lib.BOOST_FIT_MAX_ROWS} supported)")
        if m < 1:
            raise ValueError("fit needs at least one member row")
        border_list = _boost_fit.borders(Xm, border_count)
        if not any(b.size for b in border_list):
            raise ValueError("no feature has a border (every column is constant or NaN): nothing to split on")
        scores = np.zeros((m, k), dtype=np.float64)
        fit = _boost_fit.fit_host(Xm, y_idx, border_list, p, scores, device=device)
        model = cls(_boost_fit.trees_of(fit, border_list), X.shape[1], 1.0, np.zeros(k), label_mapper, thresholds, device=device)
        model.train_scores = scores
        model.borders_ = border_list
        model.n_dropped_ = n - m
        return model

    @property
    def is_trained(self):
        return len(self._depth) > 0

    @property
    def num_bcs(self) -> int:
        """fpt_base.py:37-46"""
        if self.n_classes is not None:
            return self.n_classes
        if self.label_mapper is not None:
            return len(self.label_mapper) - self.noise_class
        raise ValueError("Label mapper or n_classes not set.")

    def to_c(self) -> "_lib.BoostModelC":
        """wdx_boost_model view of the host arrays (valid while ``self`` is alive)."""
        return _lib.BoostModelC(
            int(self._depth.size), self.n_features, self.dim, self.k, self._depth.ctypes.data,
            self._split_feature.ctypes.data, self._split_border.ctypes.data, self._split_nan_true.ctypes.data,
            self._leaf_values.ctypes.data, self.scale, self._bias.ctypes.data,
            self._label_arr.ctypes.data if self.label_mapper else None,
            None if self.thresholds is None else self.thresholds.ctypes.data,
        )

    def _ensure_resident(self):
        return _own_slot(_lib.default_context(self._device), self)

    def predict_raw(self, X: np.ndarray):
        """(raw float64 (n, dim), y_prob float64 (n, k), y_pred int64 (n,), conf float64 (n,)) of ``X`` (n, n_features)."""
        if not self.is_trained:
            msg = "Model not trained."
            logging.error(msg)
            raise ValueError(msg)
        if not self.label_mapper:
            msg = "Label mapper not set."
            logging.error(msg)
            raise ValueError(msg)
        X = np.asarray(X)
        if X.ndim == 1:
            X = X.reshape(1, -1)
        if X.ndim != 2 or X.shape[1] != self.n_features:
            raise ValueError(f"X must have the model's number of features as columns  ({self.n_features}).")
        X = np.ascontiguousarray(X, dtype=np.float64)
        n = X.shape[0]
        ctx = self._ensure_resident()
        raw, y_prob = np.empty((n, self.dim), dtype=np.float64), np.empty((n, self.k), dtype=np.float64)
        y_pred, conf = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64)
        _lib.check(_lib.load().wdx_boost_predict(ctx.handle, _lib.ptr(X), n, _lib.ptr(raw), _lib.ptr(y_prob), _lib.ptr(y_pred),
                                                 _lib.ptr(conf)))
        return raw, y_prob, y_pred.astype(np.int64), conf

    def predict(self, X: np.ndarray, return_df: bool = False, **kwargs) -> Union[Tuple[np.ndarray, np.ndarray], "object"]:
        """(y_pred, conf) or the predictions DataFrame -- fpt_boost.py:14-52.  Additional arguments are accepted and ignored."""
        _, y_prob, y_pred, conf = self.predict_raw(X)
        if return_df:
            return predictions_to_df(y_pred, y_prob, conf, self.label_mapper)
        return y_pred, conf


def from_reference(model, device: Optional[int] = None):
    """Device counterpart of a loaded reference model (``warpdemux.file_proc.load_model``), by its class name."""
    name = type(model).__name__
    if name == "DTW_SVM":
        return DTW_SVM.from_reference(model, device=device)
    if name == "DTW_MLP":
        return DTW_MLP.from_reference(model, device=device)
    if name == "Fpt_Boost":
        return Fpt_Boost.from_reference(model, device=device)
    raise NotImplementedError(f"no device model for {name} (DTW_SVM, DTW_MLP and Fpt_Boost are supported)")


def _svm_cv_on_device(Xm, y_idx, classes, window, penalty, gamma, pwr_dist, C, class_weight, tol, max_iter, random_state, cv, with_full,
                      device, distances=None, targets=None):
    """What `DTW_SVM.cross_val_predict` and ``DTW_SVM.fit(thresholds="cv")`` share: D, K = exp_rule(-(gamma D^p)) in place, the one
    solve and the coupling on the device -> host arrays (and, with ``targets``, the thresholds of the out-of-fold probabilities)."""
    import torch

    from .engine import DemuxEngine

    eng = DemuxEngine(np.zeros((1, Xm.shape[1])), 15, 0.1, device=int(device) if device is not None else 0)
    try:
        with torch.cuda.device(eng.tdev):
            if distances is None:
                D = eng.self_distances(torch.tensor(Xm, device=eng.tdev), window, penalty)
            else:
                D = torch.tensor(np.ascontiguousarray(distances, dtype=np.float32), device=eng.tdev)
            K = eng.svm_kernel(D, gamma, pwr_dist, out=D)
            r = eng.svm_cross_val(K, y_idx, len(classes), C, class_weight, tol, max_iter, random_state, cv, with_full, classes=classes)
            pred_idx = r.pred_idx.cpu().numpy()
            out = {"prob": r.prob.cpu().numpy(), "conf": r.conf.cpu().numpy(), "fold": r.fold_of_row.copy(), "fit_info": r.fit_info,
                   "full": r.full, "pred": np.where(pred_idx >= 0, np.asarray(classes)[np.maximum(pred_idx, 0)], -1).astype(np.int64)}
            if targets is not None:
                thr, kept, hit, skipped = eng.accuracy_thresholds(r.prob, torch.tensor(np.asarray(y_idx, dtype=np.int32), device=eng.tdev), targets)
                out.update(thresholds=thr.cpu().numpy(), kept=kept.cpu().numpy(), hit=hit.cpu().numpy(), skipped=int(skipped))
            return out
    finally:
        eng.close()


def accuracy_thresholds(y_prob, y, label_mapper, targets=(0.99,), resolution=100, device: Optional[int] = None):
    """Per-class confidence thresholds from labelled probabilities the caller holds -- held-out rows of a `DTW_MLP` or an
    `Fpt_Boost`, say: float64 (k,) for one target, (T, k) for a sequence of them, usable as ``thresholds=`` of any of the three
    classes.  ``y_prob``: (n, k) host probabilities, columns in ``label_mapper``'s order; ``y``: the rows' true labels (a label
    ``label_mapper`` does not name, -1 for instance, leaves its row out, like a probability that is not finite);
    ``targets``: accuracies as fractions that are whole numbers of per mille (0.95, 0.999; ValueError otherwise).

    The rule is the engine's own (include/wdx.h: wdx_accuracy_thresholds_device; the reference ships threshold tables but not the
    procedure behind them): with ``conf = top1 - top2`` binned on the grid ``j / resolution``, a class's threshold is the smallest
    ``j / resolution``, j >= 1, at which the rows called that class with at least that margin are right in at least the target
    share of cases, and ``+inf`` -- no read of that class is called -- where no margin reaches it.  Runs on the device."""
    from . import _thresholds

    y_prob = np.ascontiguousarray(y_prob, dtype=np.float64)
    if y_prob.ndim != 2:
        raise ValueError(f"y_prob must be (n, k), not {y_prob.shape}")
    n, k = y_prob.shape
    mapper = {int(i): int(c) for i, c in dict(label_mapper).items()}
    if sorted(mapper) != list(range(k)):
        raise ValueError(f"label_mapper must map 0 .. {k - 1}, one entry per column of y_prob")
    y = np.asarray(y)
    if y.shape != (n,):
        raise ValueError(f"y must hold one label per row: shape ({n},), not {y.shape}")
    y_idx = np.full(n, -1, dtype=np.int32)
    for i, c in mapper.items():
        y_idx[y == c] = i
    single = np.ndim(targets) == 0
    pm = _thresholds.targets_per_mille(targets)
    thr, _, _, _ = _thresholds.host(y_prob, y_idx, pm, resolution, device=device)
    return thr[0] if single else thr
