"""MI355X counterparts of ``warpdemux.models.dtw_svm.DTW_SVM`` and ``dtw_mlp.DTW_MLP``.

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

from . import _lib


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


class _ResidentDTWModel:
    """What DTW_SVM and DTW_MLP share: the reference fingerprints, the DTW parameters and the label map on the host, the
    upload to the process's context, and ``predict``'s validation.  Subclasses name their context slot (``_owner_attr``),
    the library's setter (``_setter``) and the text of the column-mismatch error (``_column_error``)."""

    _owner_attr: str
    _setter: str

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
        L = _lib.load()
        _lib.check(L.wdx_set_refs(ctx.handle, _lib.ptr(self._X), self._X.shape[0], self._X.shape[1],
                                  int(self.window) if self.window else 0, float(self.penalty) if self.penalty else 0.0))
        if getattr(ctx, self._owner_attr, None) is not self:
            setattr(ctx, self._owner_attr, None)
            m = self.to_c()
            _lib.check(getattr(L, self._setter)(ctx.handle, C.byref(m)))
            setattr(ctx, self._owner_attr, self)
        return ctx

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

    _owner_attr, _setter = "_svm_owner", "wdx_svm_set_model"

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
    def from_reference(cls, model, device: Optional[int] = None) -> "DTW_SVM":
        """From a reference ``DTW_SVM`` instance (a loaded model_files/*.joblib)."""
        svc = model.model
        if getattr(svc, "kernel", None) != "precomputed" or not getattr(svc, "probability", False):
            raise ValueError("expected SVC(kernel='precomputed', probability=True)")
        return cls(
            _X=model._X, n_support=svc._n_support, support=svc.support_, dual_coef=svc._dual_coef_,
            rho=-np.asarray(svc._intercept_, dtype=np.float64), probA=svc._probA, probB=svc._probB,
            label_mapper=model.label_mapper, thresholds=model.thresholds, window=model.window,
            penalty=model.penalty, gamma=model.gamma, pwr_dist=model.pwr_dist, block_size=model.block_size,
            device=device,
        )

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

    _owner_attr, _setter = "_mlp_owner", "wdx_mlp_set_model"

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


def from_reference(model, device: Optional[int] = None):
    """Device counterpart of a loaded reference model (``warpdemux.file_proc.load_model``), by its class name."""
    name = type(model).__name__
    if name == "DTW_SVM":
        return DTW_SVM.from_reference(model, device=device)
    if name == "DTW_MLP":
        return DTW_MLP.from_reference(model, device=device)
    raise NotImplementedError(f"no device model for {name} (DTW_SVM and DTW_MLP are supported)")
