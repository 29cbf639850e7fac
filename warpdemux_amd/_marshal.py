"""What every host way in does between its caller's arguments and the C ABI, once: the checks of a minibatch's input arrays
(`minibatch`, `adc_rows`, `windows`, `per_read`), the result arrays of a minibatch (`outputs`, `out_addrs`, `out_c`), what a
`MinibatchPipeline` / `Feeder` / `LiveDemux` serves (`deployment`) and the two uploads (`set_refs`, `set_model`).  Everything
here runs in Python before a pointer is handed to the library: a refusal is a ``ValueError`` and touches no device.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

from . import _lib

# ---- input arrays ---------------------------------------------------------------------------------------------------------


def per_read(n: int, dtype, name: str, values):
    """C-contiguous `dtype` array of shape (n,) -- THE check of an array the library indexes by read.  It is passed by
    address, so a short one is an out-of-bounds read and a 2-D one misaligns every entry behind the first row.  `name`
    names it in the refusal."""
    v = np.ascontiguousarray(values, dtype=dtype)
    if v.shape != (n,):
        raise ValueError(f"{name} must have one entry per read")
    return v


def windows(n: int, adapter_start, adapter_end, success):
    """(a_start int32, a_end int32, ok uint8 or None) of n reads.  What the caller reads when one of them is not (n,):
    "adapter_start/adapter_end must have one entry per read", "success must have one entry per read"."""
    return (per_read(n, np.int32, "adapter_start/adapter_end", adapter_start),
            per_read(n, np.int32, "adapter_start/adapter_end", adapter_end),
            None if success is None else per_read(n, np.uint8, "success", success))


def minibatch(signals, adapter_start, adapter_end, success):
    """A (n_reads, stride) float32 minibatch (file_proc.py:244-260 layout, NaN tail) and its per-read arrays, checked:
    ``(sig, a_start, a_end, ok, n, stride)``."""
    sig = np.asarray(signals)
    if sig.ndim != 2:
        raise ValueError("signals must be a 2-D (n_reads, stride) array")
    sig = np.ascontiguousarray(sig, dtype=np.float32)
    n, stride = sig.shape
    return (sig, *windows(n, adapter_start, adapter_end, success), n, stride)


def adc_rows(adc, row_len, offset, scale, adapter_start, adapter_end, success, row_off=None, row_win=None):
    """An int16 minibatch and its per-read arrays, checked: ``(adc, n, stride, row_len, offset, scale, row_off, row_win,
    a_start, a_end, ok)``.  ``adc`` itself is never copied or converted: an array that is not C-contiguous int16 is refused
    (the point of this path is the bytes that do not move).  Without ``row_off`` it is 2-D; with it, 1-D packed rows
    (`sig_proc.adc_minibatch`) and ``stride`` is 0."""
    a = adc if isinstance(adc, np.ndarray) else np.asarray(adc)
    if a.dtype != np.int16 or not a.flags.c_contiguous:
        raise ValueError("adc must be a C-contiguous int16 array (it is passed by address, never converted)")
    r_len = np.ascontiguousarray(row_len, dtype=np.int32)
    n = int(r_len.shape[0]) if r_len.ndim == 1 else -1
    if row_off is None:
        if a.ndim != 2 or a.shape[0] != n:
            raise ValueError("adc must be a 2-D (n_reads, stride) array with one row_len per row")
        stride = int(a.shape[1])
        if row_win is not None:
            raise ValueError("row_win belongs to packed rows (row_off)")
        r_off = r_win = None
    else:
        r_off = np.ascontiguousarray(row_off, dtype=np.int64)
        if a.ndim != 1 or n < 0 or r_off.shape != (n + 1,):
            raise ValueError("packed rows: adc must be 1-D, row_off int64[n_reads + 1]")
        if n and (r_off[0] < 0 or r_off[-1] > a.shape[0] or (np.diff(r_off) < 0).any()):
            raise ValueError("packed rows: row_off must ascend within adc")
        stride = 0
        r_win = None if row_win is None else per_read(n, np.int32, "row_win", row_win)
    off, sc = per_read(n, np.float32, "offset/scale", offset), per_read(n, np.float32, "offset/scale", scale)
    return (a, n, stride, r_len, off, sc, r_off, r_win, *windows(n, adapter_start, adapter_end, success))


# ---- result arrays --------------------------------------------------------------------------------------------------------

WANT_TAIL = _lib.WANT_SVM | _lib.WANT_BOOST      # prob / pred / conf of whichever classifier tail the context holds

# wdx_minibatch_out, = the output tail of wdx_feeder_job[_adc], in field order: (name, the WDX_WANT_* bits that ask for it;
# None: every minibatch brings it back)
_OUT = (("status", None), ("call", None), ("dist", _lib.WANT_DIST), ("fpt", _lib.WANT_FPT), ("dwell", _lib.WANT_DWELL),
        ("stats", _lib.WANT_STATS), ("prob", WANT_TAIL), ("pred", WANT_TAIL), ("conf", WANT_TAIL))


def outputs(n: int, K: int, nY: int, n_classes: int, want: int) -> dict:
    """The result arrays of a minibatch of n reads by name, None where `want` (WDX_WANT_* bits) does not ask: K events per
    fingerprint, nY references, n_classes columns of the classifier tail.  ``pred`` is int32 as the library writes it;
    callers hand out ``astype(np.int64)``."""
    tail = want & WANT_TAIL
    return {
        "status": np.empty(n, dtype=np.int32),
        "call": np.empty(n, dtype=np.int32),
        "dist": np.empty((n, nY), dtype=np.float32) if want & _lib.WANT_DIST else None,
        "fpt": np.empty((n, K), dtype=np.float64) if want & _lib.WANT_FPT else None,
        "dwell": np.empty((n, K), dtype=np.int64) if want & _lib.WANT_DWELL else None,
        "stats": np.empty((n, 6), dtype=np.float64) if want & _lib.WANT_STATS else None,
        "prob": np.empty((n, n_classes), dtype=np.float64) if tail else None,
        "pred": np.empty(n, dtype=np.int32) if tail else None,
        "conf": np.empty(n, dtype=np.float64) if tail else None,
        "refine_idx": np.empty((n, 3), dtype=np.int32) if want & _lib.WANT_REFINE_IDX else None,
    }


def out_addrs(o: dict, want: int = ~0) -> list:
    """The nine addresses of wdx_minibatch_out / of a feeder job's output tail; ``want`` narrows arrays that were allocated
    for more (a `LiveDemux` allocates once, for its capacity and every bit)."""
    return [_lib.addr(o[k]) if bit is None or want & bit else None for k, bit in _OUT]


def out_c(o: dict, want: int = ~0) -> "_lib.MinibatchOutC":
    return _lib.MinibatchOutC(*out_addrs(o, want))


# ---- what an object serves ------------------------------------------------------------------------------------------------

_KINDS = (("DTW_SVM", _lib.LIVE_TAIL_SVM, "wdx_svm_set_model"), ("DTW_MLP", _lib.LIVE_TAIL_MLP, "wdx_mlp_set_model"),
          ("Fpt_Boost", _lib.LIVE_TAIL_BOOST, "wdx_boost_set_model"))
_NAME = {kind: name for name, kind, _ in _KINDS}
_DTW = (_lib.LIVE_TAIL_SVM, _lib.LIVE_TAIL_MLP)    # tails on the distances to the model's own ``_X``


def model_kind(model) -> int:
    """WDX_LIVE_TAIL_* of a `models` object (None: no tail), -1 for anything else."""
    from . import models

    if model is None:
        return _lib.LIVE_TAIL_NONE
    return next((kind for name, kind, _ in _KINDS if isinstance(model, getattr(models, name))), -1)


class Deployment(NamedTuple):
    refs: np.ndarray            # (nY, K) float64, C-contiguous; (0, K) without references
    window: Optional[int]
    penalty: Optional[float]
    nY: int
    K: int                      # events per fingerprint = reference length = a boost model's n_features
    params: object              # sig_proc.SegParams
    kind: int                   # WDX_LIVE_TAIL_* of the model
    n_classes: int              # columns of the tail's prob (0 without a model)


def refine_options(refine, long_windows: bool, who: str) -> bool:
    """``refine.optimal_cpts`` of an object that owns its context, checked against ``long_windows`` before the context exists."""
    on = bool(getattr(refine, "optimal_cpts", False))
    if on and long_windows:
        raise ValueError(f"{who}: optimal_cpts and long_windows do not go together (WDX_OPT_REFINE_OPTIMAL_CPTS serves adapter "
                         "windows of up to MAX_ADAPTER_SAMPLES samples)")
    return on


def wide_dtw_option(wide_dtw, who: str) -> bool:
    """The ``wide_dtw=`` keyword of an object that owns its context (WDX_OPT_WIDE_DTW), checked before the context exists: a
    bool and nothing else -- an integer window handed to the wrong keyword must not switch a kernel."""
    if not isinstance(wide_dtw, (bool, np.bool_)):
        raise ValueError(f"{who}: wide_dtw is True or False, not {wide_dtw!r}")
    return bool(wide_dtw)


def deployment(refs, window, penalty, params, model, refine, *, who: str, models: tuple, nothing_to_serve: str,
               bare_refine: bool, refine_dtw: bool) -> Deployment:
    """THE rule of what a `MinibatchPipeline`, `Feeder` or `LiveDemux` serves, checked before any context exists
    (``ValueError``).  The references are ``refs`` or a DTW model's ``_X`` (with its window and penalty), never both; they may
    be missing only behind an `Fpt_Boost`, which classifies the fingerprints themselves, or -- fingerprints only -- with
    ``refine``.  K is ``refine.barcode_keep_events`` under refinement, else ``params.barcode_num_events``, which defaults to
    the reference length, else to the boost model's ``n_features``; it must equal both.

    What the class serves is its own statement: ``who`` (its name) takes the model classes named in ``models``, refuses
    having neither references nor a model that does without with ``nothing_to_serve``, serves ``refine`` without either if
    ``bare_refine`` and ``refine`` in front of a DTW model if ``refine_dtw``."""
    from .sig_proc import RefineParams, SegParams

    kind = model_kind(model)
    if model is not None and _NAME.get(kind) not in models:
        names = ", ".join(models[:-1]) + " and " + models[-1] if len(models) > 1 else models[0]
        raise ValueError(f"{who} serves models.{names}, not {type(model).__name__}")
    if kind in _DTW:
        if refs is not None:
            raise ValueError("pass either refs or model (whose _X are the references)")
        refs, window, penalty = model._X, model.window, model.penalty
    if refine is not None:
        if not isinstance(refine, RefineParams) or refine.query is None or np.size(refine.query) == 0:
            raise ValueError("refine must be a sig_proc.RefineParams with a consensus query")
        if kind in _DTW and not refine_dtw:
            raise ValueError(f"consensus refinement is served without a model or with an Fpt_Boost, not with a {type(model).__name__}")
    if refs is None:
        if kind != _lib.LIVE_TAIL_BOOST and not (bare_refine and refine is not None):
            raise ValueError(nothing_to_serve)
        ref_len = None
    else:
        refs = np.ascontiguousarray(refs, dtype=np.float64)
        if refs.ndim != 2:
            raise ValueError("refs must be (nY, K)")
        ref_len = int(refs.shape[1])
    if refine is not None:
        K, k_name = int(refine.barcode_keep_events), "refine.barcode_keep_events"
        params = params or SegParams(barcode_num_events=K)    # (the library runs a refine minibatch with K = keep events)
    else:
        params = params or SegParams(barcode_num_events=ref_len if ref_len is not None else int(model.n_features))
        K, k_name = int(params.barcode_num_events), "barcode_num_events"
    if ref_len is not None and K != ref_len:
        raise ValueError(f"{k_name} ({K}) must equal the reference length ({ref_len})")
    if kind == _lib.LIVE_TAIL_BOOST and K != int(model.n_features):
        raise ValueError(f"the boost model takes {int(model.n_features)} features: {k_name} ({K}) must equal the boost model's "
                         f"n_features ({int(model.n_features)})")
    if refs is None:
        refs = np.zeros((0, K), dtype=np.float64)
    n_classes = 0 if model is None else int(model.n_classes if kind == _lib.LIVE_TAIL_SVM else model.k)
    return Deployment(refs, window, penalty, int(refs.shape[0]), K, params, kind, n_classes)


# ---- uploads --------------------------------------------------------------------------------------------------------------


def set_refs(ctx, refs, window, penalty):
    """`refs` ((nY, K) float64, C-contiguous) become the context's reference set (the library compares a content hash and
    uploads only on change); a missing window / penalty goes to the library as 0."""
    _lib.check(_lib.load().wdx_set_refs(ctx.handle, _lib.ptr(refs), refs.shape[0], refs.shape[1],
                                        int(window) if window else 0, float(penalty) if penalty else 0.0))


def set_model(ctx, model):
    """`model` (a `models.DTW_SVM`, `DTW_MLP` or `Fpt_Boost`) into its slot of the context, by the setter of its class."""
    setter = {kind: s for _, kind, s in _KINDS}.get(model_kind(model))
    if setter is None:
        raise ValueError(f"no device model for {type(model).__name__} (DTW_SVM, DTW_MLP and Fpt_Boost are supported)")
    m = model.to_c()     # a view of the model's host arrays: the library copies what it needs during the call
    _lib.check(getattr(_lib.load(), setter)(ctx.handle, C.byref(m)))
