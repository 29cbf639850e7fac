"""Many worker processes, ONE GPU-facing process: the drop-in for the reference's `-j 8..16` forked workers
(file_proc.py:1197-1243: a ProcessPoolExecutor whose workers each run fingerprint + model on their minibatches,
file_proc.py:380-454).

Sixteen processes that each drive the GPU through their own context run at 40 % of the rate of four (the device
time-slices the processes' queues).  Here the PARENT creates a `Feeder` before it forks its workers: a ring of
minibatch slots in shared memory plus one forked process that owns the engine context, page-locks the ring and keeps
up to eight minibatches in flight (`wdx_feeder_serve`).  A worker's call copies the adapter windows of its minibatch
into a free slot and sleeps until the results are there (`wdx_feeder_run`: no context, no HIP call in the worker).

What comes back is what the reference's worker needs from a minibatch (file_proc.py:418-450):

* `fingerprint_batch(...)` -> `sig_proc.FingerprintBatch` (fingerprint, dwell times, six statistics, status): the
  ReadResults `save_fpts_signals` / `save_detected_boundaries` take (file_proc.py:707-754), = `sig_proc.fingerprint_batch`;
* `predict(X, return_df=...)` -> what `DTW_SVM.predict` returns (models/dtw_svm.py:54-98) for fingerprints the worker holds;
* `detect_and_predict(...)` -> both from ONE pass over the rows (the fingerprints never leave the device between the two);
* `demux_batch(...)` -> `sig_proc.DemuxBatch` (status, nearest-reference call, distance rows), = `sig_proc.demux_batch`.

    feeder = Feeder(model=DTW_SVM.from_reference(model), params=SegParams.from_spc(spc), max_reads=1000, stride=10000)
    with ProcessPoolExecutor(P, mp_context=multiprocessing.get_context("fork")) as pool:   # workers inherit `feeder`
        ... in a worker:  fb, preds = feeder.detect_and_predict(minibatch, adapter_start, adapter_end, success, return_df=True)
    feeder.close()

``Feeder(..., refine=RefineParams(...))`` serves the tRNA models' consensus-refinement branch (the ring keeps the
refinement parameters and the consensus query): `fingerprint_batch[_adc]` then returns what
`sig_proc.fingerprint_refine_batch` returns, ``refine_idx`` included, and `sig_proc.read_results_from_batch(fb, drs, ids,
refined=True)` makes the reference's ReadResults of it.  Such a feeder may be created without references
(``refs=None, model=None``) and then serves the fingerprints only.

``Feeder(model=Fpt_Boost, refs=None, refine=..., adc=...)`` serves the tRNA models' classifier as well
(`models.Fpt_Boost`, resident on the feeder's context; WDX_WANT_BOOST): `detect_and_predict[_adc]` and `predict` return
what they return for a `DTW_SVM` -- the ReadResult arrays and the prediction from ONE pass, no references needed.

A worker that dies while it holds a slot does not cost the ring that slot, and a feeder process that dies is noticed
by the workers (`WdxNoDevice`) even while it is a zombie nobody has reaped (wdx_feeder.hip).
"""
from __future__ import annotations

import ctypes as C
import multiprocessing as mp
import os
from multiprocessing import shared_memory
from typing import Optional

import numpy as np

from . import _lib, _marshal
from .sig_proc import DemuxBatch, FingerprintBatch, RefineParams, SegParams, fingerprints

MAX_SLOTS = 32      # ring slots (WDX_FEEDER_MAX_RING_SLOTS); the feeder keeps at most 8 of them in flight on the device


def _serve(shm_name: str, refs, window, penalty, model, device: int, ready, long_windows: bool = False, optimal_cpts: bool = False,
           wide_dtw: bool = False):
    """The GPU-facing process (forked from a parent that never touched the GPU)."""
    shm = shared_memory.SharedMemory(name=shm_name)
    rc = 1
    try:
        L = _lib.load()
        ctx = _lib.Context(device)
        if long_windows:
            ctx.set_long_windows()   # (OPT_LONG_WINDOWS and OPT_LONG_REFINE_WINDOWS: a refine ring looks at the second)
        if optimal_cpts:    # (refine.optimal_cpts: the ring's refine minibatches are cut at their optimal change-points)
            ctx.set_option(_lib.OPT_REFINE_OPTIMAL_CPTS, 1)
        if wide_dtw:
            ctx.set_option(_lib.OPT_WIDE_DTW, 1)
        if refs.shape[0]:   # (a fingerprint-only refine ring has none)
            _marshal.set_refs(ctx, refs, window, penalty)
        if model is not None:
            _marshal.set_model(ctx, model)
        base = C.addressof(C.c_char.from_buffer(shm.buf))
        # (wdx_feeder_serve announces itself in the ring -- server_pid + heartbeat -- once the ring is page-locked; the
        # parent polls wdx_feeder_alive after this event)
        ready.set()
        _lib.check(L.wdx_feeder_serve(ctx.handle, C.c_void_p(base)))
        ctx.close()
        rc = 0
    except BaseException:  # noqa: BLE001  (reported through the exit code and stderr; the ring is stopped below)
        import sys
        import traceback

        traceback.print_exc(file=sys.stderr)
        try:
            base = C.addressof(C.c_char.from_buffer(shm.buf))
            _lib.load().wdx_feeder_stop(C.c_void_p(base))
        except Exception:  # noqa: BLE001
            pass
        ready.set()
    finally:
        os._exit(rc)   # (no interpreter teardown in the forked child: the parent owns the shared memory)


class Feeder:
    """Create in the parent BEFORE forking the workers (the parent itself makes no GPU call); the workers use the
    inherited object.  `max_reads` x `stride` = the largest minibatch a slot holds (file_proc's 1000 x sig_preload_size).

    Either `refs` (+ `window`, `penalty`): nearest-reference calls only -- or `model`, a `warpdemux_amd.models.DTW_SVM`
    (`DTW_SVM.from_reference(loaded_model)`): its `_X` are the references and `predict` / `detect_and_predict` are served.

    ``adc=True``: the ring's slots hold int16 ADC samples and the workers call `fingerprint_batch_adc` /
    `demux_batch_adc` / `detect_and_predict_adc` with the raw samples and ``row_len`` / ``offset`` / ``scale`` per read --
    half the bytes in the worker's copy, in the ring and over the bus; the device calibrates by the formula of
    `sig_proc.calibrate_adc`, and the results are those of the float32 calls on its rows, bit for bit.  The float32 calls
    are refused on such a ring, and the ``*_adc`` calls on a float32 ring.

    ``refine``: every minibatch takes the consensus-refinement branch with these parameters (K =
    ``refine.barcode_keep_events``); with it, and only with it, ``refs`` and ``model`` may both be None: a fingerprint-only
    feeder, on which `demux_batch`, `detect_and_predict` and `predict` are refused.

    ``model`` may also be a `warpdemux_amd.models.Fpt_Boost` (the tRNA models): it classifies the fingerprints themselves, so
    ``refs`` may be None with or without ``refine`` (`demux_batch` is then refused) or given beside it; K must equal
    ``model.n_features``.

    ``long_windows``: the serving context fingerprints adapter windows of up to 65 536 samples (WDX_OPT_LONG_WINDOWS, and
    WDX_OPT_LONG_REFINE_WINDOWS for a ``refine`` ring -- `stride` must hold such rows).

    ``wide_dtw``: the serving context runs effective windows 33 .. L (``window=None`` on fingerprints of 33 .. 256 events) on
    the wide-window DTW kernel instead of the scratch rows (WDX_OPT_WIDE_DTW); same results."""

    def __init__(self, refs=None, window=None, penalty=None, params: Optional[SegParams] = None, max_reads: int = 1000,
                 stride: int = 10000, n_slots: int = 16, device: int = 0, start_timeout: float = 120.0, model=None,
                 adc: bool = False, refine: Optional[RefineParams] = None, long_windows: bool = False,
                 wide_dtw: bool = False):
        wide_dtw = _marshal.wide_dtw_option(wide_dtw, "Feeder")
        optimal = _marshal.refine_options(refine, long_windows, "Feeder")
        d = _marshal.deployment(refs, window, penalty, params, model, refine, who="Feeder", models=("DTW_SVM", "Fpt_Boost"),
                                bare_refine=True, refine_dtw=True, nothing_to_serve="refs or model is required")
        if not 1 <= int(n_slots) <= MAX_SLOTS:
            raise ValueError(f"n_slots must be in [1, {MAX_SLOTS}]")
        self.boost = d.kind == _lib.LIVE_TAIL_BOOST     # an Fpt_Boost: no references of its own
        self.refine, self.model, self.params, self.nY, self.K, self.n_classes = refine, model, d.params, d.nY, d.K, d.n_classes
        self._tail = _lib.WANT_BOOST if self.boost else _lib.WANT_SVM
        self.label_mapper = dict(model.label_mapper) if model is not None else None
        self.max_reads, self.stride, self.n_slots = int(max_reads), int(stride), int(n_slots)
        self.L = _lib.load()
        self.adc = bool(adc)
        geo = _lib.FeederGeometryC(self.n_slots, self.K, self.n_classes,
                                   _lib.FEEDER_SAMPLES_INT16 if self.adc else _lib.FEEDER_SAMPLES_FLOAT32, self.max_reads,
                                   self.stride, self.nY)
        pc = self.params.to_c()
        rc = refine.to_c() if refine is not None else None
        nbytes = int((self.L.wdx_feeder_ring_bytes if rc is None else self.L.wdx_feeder_ring_bytes_refine)(C.byref(geo)))
        if nbytes == 0:
            raise ValueError("bad ring geometry")
        self._shm = self._proc = None
        shm = shared_memory.SharedMemory(create=True, size=nbytes)
        base = C.addressof(C.c_char.from_buffer(shm.buf))
        init = (self.L.wdx_feeder_ring_init(C.c_void_p(base), nbytes, C.byref(geo), C.byref(pc)) if rc is None else
                self.L.wdx_feeder_ring_init_refine(C.c_void_p(base), nbytes, C.byref(geo), C.byref(pc), C.byref(rc)))
        if init != _lib.WDX_SUCCESS:   # (a refused ring -- e.g. a query beyond 96 points -- leaves no shared memory behind)
            try:
                shm.close()
            except BufferError:
                pass
            shm.unlink()
            _lib.check(init)
        self._shm, self._owner, self._base = shm, os.getpid(), base
        ctx = mp.get_context("fork")
        ready = ctx.Event()
        self._proc = ctx.Process(target=_serve, args=(self._shm.name, d.refs, d.window, d.penalty, model, int(device), ready, bool(long_windows), optimal, wide_dtw),
                                 daemon=True)
        self._proc.start()
        import time

        up = ready.wait(start_timeout)
        t_end = time.monotonic() + 30.0
        while up and self._proc.is_alive() and self.L.wdx_feeder_alive(C.c_void_p(self._base)) != 1 and time.monotonic() < t_end:
            time.sleep(0.002)      # context, references, page-locking the ring: the feeder is up when it says so in the ring
        if not up or not self._proc.is_alive() or self.L.wdx_feeder_alive(C.c_void_p(self._base)) != 1:
            self.close()
            raise _lib.WdxError("the feeder process did not come up (see its stderr)")

    # ---- one minibatch ------------------------------------------------------------------------------------------------
    def _run(self, signals, adapter_start, adapter_end, success, want: int):
        sig, a_s, a_e, ok, n, stride = _marshal.minibatch(signals, adapter_start, adapter_end, success)
        out = self._outputs(n, want)
        job = _lib.FeederJobC(_lib.addr(sig), n, stride, _lib.addr(a_s), _lib.addr(a_e), _lib.addr(ok), int(want), 0,
                              *_marshal.out_addrs(out))
        if want & _lib.WANT_REFINE_IDX:
            _lib.check(self.L.wdx_feeder_run_refine(C.c_void_p(self._base), C.byref(job), None, _lib.ptr(out["refine_idx"])))
        else:
            _lib.check(self.L.wdx_feeder_run(C.c_void_p(self._base), C.byref(job)))
        return out

    def _outputs(self, n: int, want: int) -> dict:
        if want & _marshal.WANT_TAIL and self.model is None:
            raise ValueError("this feeder was created without a model (Feeder(model=DTW_SVM...))")
        return _marshal.outputs(n, self.K, self.nY, self.n_classes, want)

    def _fpt_want(self) -> int:
        """the ReadResult arrays of a minibatch; on a refine feeder with refine_idx.  A plain minibatch without references
        is legal with WDX_WANT_BOOST only (wdx_demux_submit_ex), so a boost feeder without references and without ``refine``
        always asks for the tail; `fingerprint_batch[_adc]` leaves its prediction behind."""
        return (_lib.WANT_FPT | _lib.WANT_DWELL | _lib.WANT_STATS |
                (_lib.WANT_REFINE_IDX if self.refine is not None else 0) |
                (_lib.WANT_BOOST if self.boost and self.refine is None and self.nY == 0 else 0))

    def _need_refs(self, what: str):
        if self.nY == 0:
            raise ValueError(f"{what} needs references or a DTW model: this feeder is fingerprint-only"
                             + (" behind its boost model" if self.boost else " (Feeder(refine=...))"))

    def _run_adc(self, adc, row_len, offset, scale, adapter_start, adapter_end, success, want: int):
        """One int16 minibatch through wdx_feeder_run_adc.  Shapes and dtypes of EVERY array, `success` included, are
        checked before anything is passed by address; `adc` must be a C-contiguous 2-D int16 array (it is never copied
        here; a ring's slots hold rows, not packed reads)."""
        a, n, stride, r_len, off, sc, _, _, a_s, a_e, ok = _marshal.adc_rows(adc, row_len, offset, scale, adapter_start,
                                                                             adapter_end, success)
        out = self._outputs(n, want)
        job = _lib.FeederJobAdcC(_lib.addr(a), n, stride, _lib.addr(r_len), _lib.addr(off), _lib.addr(sc), _lib.addr(a_s),
                                 _lib.addr(a_e), _lib.addr(ok), int(want), 0, *_marshal.out_addrs(out))
        if want & _lib.WANT_REFINE_IDX:
            _lib.check(self.L.wdx_feeder_run_refine(C.c_void_p(self._base), None, C.byref(job), _lib.ptr(out["refine_idx"])))
        else:
            _lib.check(self.L.wdx_feeder_run_adc(C.c_void_p(self._base), C.byref(job)))
        return out

    def demux_batch_adc(self, adc, row_len, offset, scale, adapter_start, adapter_end, success=None,
                        want_dist: bool = True) -> DemuxBatch:
        """`demux_batch` for an int16 ADC minibatch (a ``Feeder(adc=True)``)."""
        self._need_refs("demux_batch_adc")
        o = self._run_adc(adc, row_len, offset, scale, adapter_start, adapter_end, success, _lib.WANT_DIST if want_dist else 0)
        return DemuxBatch(o["status"], o["call"], o["dist"], None)

    def fingerprint_batch_adc(self, adc, row_len, offset, scale, adapter_start, adapter_end, success=None) -> FingerprintBatch:
        """`fingerprint_batch` for an int16 ADC minibatch (a ``Feeder(adc=True)``)."""
        o = self._run_adc(adc, row_len, offset, scale, adapter_start, adapter_end, success, self._fpt_want())
        return fingerprints(o)

    def detect_and_predict_adc(self, adc, row_len, offset, scale, adapter_start, adapter_end, success=None,
                               return_df: bool = False):
        """`detect_and_predict` for an int16 ADC minibatch (a ``Feeder(adc=True)``): the reference worker's whole
        minibatch from the raw samples the pod5 file holds."""
        o = self._run_adc(adc, row_len, offset, scale, adapter_start, adapter_end, success, self._fpt_want() | self._tail)
        return self._fpt_and_predictions(o, return_df)

    def demux_batch(self, signals, adapter_start, adapter_end, success=None, want_dist: bool = True) -> DemuxBatch:
        """Status, nearest-reference call and (optionally) the distance rows -- `sig_proc.demux_batch`'s result, bit for
        bit.  Callable from any process that inherited this object; blocks until the results are there."""
        self._need_refs("demux_batch")
        o = self._run(signals, adapter_start, adapter_end, success, _lib.WANT_DIST if want_dist else 0)
        return DemuxBatch(o["status"], o["call"], o["dist"], None)

    def fingerprint_batch(self, signals, adapter_start, adapter_end, success=None) -> FingerprintBatch:
        """`sig_proc.fingerprint_batch`'s result (fingerprints, dwell times, the six statistics, status), bit for bit:
        what `sig_proc.read_results_from_batch` turns into the reference's ReadResult records.  On a refine feeder:
        `sig_proc.fingerprint_refine_batch`'s result, ``refine_idx`` included."""
        o = self._run(signals, adapter_start, adapter_end, success, self._fpt_want())
        return fingerprints(o)

    def detect_and_predict(self, signals, adapter_start, adapter_end, success=None, return_df: bool = False):
        """The two halves of the reference worker's minibatch (file_proc.py:418-450) from one pass over the rows:
        `(FingerprintBatch, predictions)` with predictions = `(y_pred, y_prob)` or, with ``return_df``, the predictions
        DataFrame of `DTW_SVM.predict(np.vstack(fpts), return_df=True)` -- one row per SUCCESSFUL read, in read order,
        like the reference, which only ever shows the model the successful fingerprints."""
        o = self._run(signals, adapter_start, adapter_end, success, self._fpt_want() | self._tail)
        return self._fpt_and_predictions(o, return_df)

    def _fpt_and_predictions(self, o: dict, return_df: bool):
        fb = fingerprints(o)
        okr = o["status"] == 0
        y_pred, y_prob, conf = o["pred"][okr].astype(np.int64), o["prob"][okr], o["conf"][okr]
        if return_df:
            from .models import predictions_to_df

            return fb, predictions_to_df(y_pred, y_prob, conf, self.label_mapper)
        return fb, (y_pred, y_prob)

    def predict(self, X, return_df: bool = False):
        """`DTW_SVM.predict` (models/dtw_svm.py:54-98) through the feeder: (y_pred, y_prob) or the predictions DataFrame;
        with an `Fpt_Boost` model the same two from `wdx_feeder_predict_boost`."""
        if self.model is None:
            raise ValueError("this feeder was created without a model (Feeder(model=DTW_SVM...))")
        X = np.asarray(X)
        if X.ndim == 1:
            X = X.reshape(1, -1)
        if X.shape[1] != self.K:
            raise ValueError(f"X must have the same number of columns as the training data  ({self.K}).")
        X = np.ascontiguousarray(X, dtype=np.float64)
        n = X.shape[0]
        y_prob = np.empty((n, self.n_classes), dtype=np.float64)
        y_pred = np.empty(n, dtype=np.int32)
        conf = np.empty(n, dtype=np.float64)
        call = self.L.wdx_feeder_predict_boost if self.boost else self.L.wdx_feeder_predict
        _lib.check(call(C.c_void_p(self._base), _lib.ptr(X), n, _lib.ptr(y_prob), _lib.ptr(y_pred), _lib.ptr(conf)))
        y_pred = y_pred.astype(np.int64)
        if return_df:
            from .models import predictions_to_df

            return predictions_to_df(y_pred, y_prob, conf, self.label_mapper)
        return y_pred, y_prob

    # ---- housekeeping -------------------------------------------------------------------------------------------------
    def alive(self) -> bool:
        """True while the feeder process serves the ring."""
        return self._base is not None and self.L.wdx_feeder_alive(C.c_void_p(self._base)) == 1

    def served(self) -> int:
        v = C.c_int64(0)
        _lib.check(self.L.wdx_feeder_served(C.c_void_p(self._base), C.byref(v)))
        return int(v.value)

    def stats(self) -> dict:
        """{'served': minibatches handed back, 'reclaimed': slots taken back from dead workers, 'free_slots': now}"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        _lib.check(self.L.wdx_feeder_stats(C.c_void_p(self._base), C.byref(a), C.byref(b), C.byref(c)))
        return {"served": int(a.value), "reclaimed": int(b.value), "free_slots": int(c.value), "n_slots": self.n_slots}

    def close(self):
        """Parent only: stop the feeder process and release the ring."""
        if self._shm is None or os.getpid() != self._owner:
            return
        try:
            self.L.wdx_feeder_stop(C.c_void_p(self._base))
        except Exception:  # noqa: BLE001
            pass
        if self._proc is not None:
            self._proc.join(30)
            if self._proc.is_alive():
                self._proc.terminate()
                self._proc.join(10)
        self._base = None
        shm, self._shm = self._shm, None
        try:
            shm.close()
        except BufferError:   # (ctypes views of the buffer are still referenced somewhere: unlink regardless)
            pass
        shm.unlink()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
