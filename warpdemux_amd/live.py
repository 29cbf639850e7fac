"""Live path (BASELINE config 5): the reads of one 100 ms chunk round in one device call.

The reference runs two per-read worker loops (live_balancing/worker.py): ``segmentation_worker`` (:26-96 --
extract_adapter(0, polya_start), median/MAD clip, segment_signal, normalize, keep the last K events) and
``classification_worker`` (:99-131 -- ``model = load_model(config.model_name)``, ``model.predict(fpt, nproc=1)``).  Here

* :class:`LiveDemux` owns one engine context per thread (its own HIP stream and page-locked staging
  buffers) and turns a tick's reads into fingerprints, distances, calls and -- with a model -- class
  probabilities with ONE C-ABI call (``wdx_live_tick_ex``).  Every model kind ``load_model`` returns is served:
  ``DTW_SVM`` and ``DTW_MLP`` (DTW against the model's references, then the tail on the distances) and ``Fpt_Boost``
  (the tRNA models: consensus-refined fingerprints -- pass ``refine`` -- then the trees on the fingerprints; no
  references needed).  Rows come as float32 (:meth:`LiveDemux.tick`) or as the int16 ADC samples MinKNOW delivers, with
  each read's calibration (:meth:`LiveDemux.tick_adc`: 2 bytes per sample over the bus, calibrated on the device);
* :func:`demux_worker` is the queue-to-queue mirror of the two reference workers: it drains whatever
  ``ReadObject``s the session queued during the tick, processes them as one batch and emits them with the
  fields the reference's ``balance_worker`` reads (``data_arr`` = ``y_prob.reshape(1, -1)``, ``is_outlier``,
  two ``time_per_step`` entries).

One LiveDemux per worker thread (live_balancing/session.py:162-169 starts thread pools): calls through
different contexts overlap on the device.
"""
from __future__ import annotations

import ctypes as C
import queue as _queue
import time
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .sig_proc import RefineParams, SegParams


@dataclass
class TickResult:
    status: np.ndarray              # (n,) int32 WDX_READ_*
    call: np.ndarray                # (n,) int32 nearest reference, -1 for failed reads (and without references)
    dist: Optional[np.ndarray]      # (n, nY) float32 (NaN rows for failed reads)
    fpt: Optional[np.ndarray]       # (n, K) float64
    prob: Optional[np.ndarray]      # (n, k) float64 -- y_prob of the model's predict (with a model)
    pred: Optional[np.ndarray]      # (n,) int64 barcode label, -1 = outlier / failed read (with a model)
    conf: Optional[np.ndarray]      # (n,) float64 top1 - top2 margin (with a model)
    dwell: Optional[np.ndarray] = None        # (n, K) int64 (want_dwell)
    stats: Optional[np.ndarray] = None        # (n, 6) float64, order of sig_proc.FingerprintBatch.stats (want_stats)
    refine_idx: Optional[np.ndarray] = None   # (n, 3) int32 seg_cons_query_start / _end, sig_barcode_start (want_refine_idx)


def _model_kind(model) -> int:
    from . import models

    if model is None:
        return _lib.LIVE_TAIL_NONE
    if isinstance(model, models.DTW_SVM):
        return _lib.LIVE_TAIL_SVM
    if isinstance(model, models.DTW_MLP):
        return _lib.LIVE_TAIL_MLP
    if isinstance(model, models.Fpt_Boost):
        return _lib.LIVE_TAIL_BOOST
    raise ValueError(f"LiveDemux serves models.DTW_SVM, DTW_MLP and Fpt_Boost, not {type(model).__name__}")


_DT = {np.float32: np.dtype(np.float32), np.int16: np.dtype(np.int16)}
_SETTER = {_lib.LIVE_TAIL_SVM: "wdx_svm_set_model", _lib.LIVE_TAIL_MLP: "wdx_mlp_set_model",
           _lib.LIVE_TAIL_BOOST: "wdx_boost_set_model"}


class LiveDemux:
    """``refs``: (nY, K) reference fingerprints, or pass ``model``:

    * a :class:`warpdemux_amd.models.DTW_SVM` or ``DTW_MLP``: its ``_X``/window/penalty become the references and its
      classifier tail runs on the device too;
    * a :class:`warpdemux_amd.models.Fpt_Boost`: its trees run on the fingerprints themselves.  ``refs`` may be ``None``
      (``call`` is -1 for every read, there are no distances); with ``refs`` the nearest-reference call and the distances
      come back beside the model's answer.

    ``refine``: a :class:`warpdemux_amd.sig_proc.RefineParams` selects the consensus-refinement branch (the tRNA models
    were trained on refined fingerprints); K is then ``refine.barcode_keep_events``.  It is served without a model or
    with an ``Fpt_Boost`` -- no DTW model is trained on refined fingerprints.

    ``adc``: :meth:`tick_adc` works on ANY LiveDemux; ``adc=True`` only makes the constructor's warm-up tick an int16 one,
    so that the int16 staging buffers too are allocated before the run starts.

    Every check of the arguments happens before a context is created and raises ``ValueError``."""

    def __init__(self, refs=None, window=None, penalty=None, params: Optional[SegParams] = None, *, model=None,
                 refine: Optional[RefineParams] = None, adc: bool = False, device: int = 0, max_reads: int = 512,
                 max_samples: int = 10000):
        self.tail = _model_kind(model)
        self.model = model
        if self.tail in (_lib.LIVE_TAIL_SVM, _lib.LIVE_TAIL_MLP):
            refs, window, penalty = model._X, model.window, model.penalty
        if refine is not None:
            if not isinstance(refine, RefineParams) or refine.query is None or np.size(refine.query) == 0:
                raise ValueError("refine must be a sig_proc.RefineParams with a consensus query")
            if self.tail in (_lib.LIVE_TAIL_SVM, _lib.LIVE_TAIL_MLP):
                raise ValueError("consensus refinement is served without a model or with an Fpt_Boost, not with a "
                                 f"{type(model).__name__}")
        if refs is None:
            if self.tail != _lib.LIVE_TAIL_BOOST:
                raise ValueError("refs may only be None with an Fpt_Boost model (its tail needs no references)")
            self.nY, ref_len = 0, None
        else:
            refs = np.ascontiguousarray(refs, dtype=np.float64)
            if refs.ndim != 2:
                raise ValueError("refs must be (nY, K)")
            self.nY, ref_len = refs.shape
        if refine is not None:
            self.K, k_name = int(refine.barcode_keep_events), "refine.barcode_keep_events"
            self.params = params or SegParams()
        else:
            default_k = ref_len if ref_len is not None else model.n_features
            self.params = params or SegParams(barcode_num_events=default_k)
            self.K, k_name = int(self.params.barcode_num_events), "barcode_num_events"
        if ref_len is not None and self.K != ref_len:
            raise ValueError(f"{k_name} ({self.K}) must equal the reference length ({ref_len})")
        if self.tail == _lib.LIVE_TAIL_BOOST and self.K != model.n_features:
            raise ValueError(f"{k_name} ({self.K}) must equal the boost model's n_features ({model.n_features})")
        self.refine = refine
        self._pc = self.params.to_c()
        self._rc = None if refine is None else refine.to_c()
        self.k = 0 if model is None else (model.n_classes if self.tail == _lib.LIVE_TAIL_SVM else model.k)

        self.L = _lib.load()
        self.ctx = _lib.Context(device)      # this object's own context = own stream + staging buffers
        if refs is not None:
            _lib.check(self.L.wdx_set_refs(self.ctx.handle, _lib.ptr(refs), self.nY, ref_len,
                                           int(window) if window else 0, float(penalty) if penalty else 0.0))
        if model is not None:
            self._m = model.to_c()
            _lib.check(getattr(self.L, _SETTER[self.tail])(self.ctx.handle, C.byref(self._m)))
        self._cap = 0
        self._reserve(max_reads)
        # first tick at full size now: staging buffers and workspaces are allocated before the run starts
        if max_reads > 0 and max_samples > 0:
            a_s, a_e = np.zeros(max_reads, np.int32), np.full(max_reads, max_samples, np.int32)
            if adc:
                z = np.zeros(max_samples, dtype=np.int16)
                self.tick_adc([z] * max_reads, np.zeros(max_reads, np.float32), np.ones(max_reads, np.float32), a_s, a_e)
            else:
                z = np.zeros(max_samples, dtype=np.float32)
                self.tick([z] * max_reads, a_s, a_e)

    def _reserve(self, n):
        if n <= self._cap:
            return
        self._cap = n
        self._rows = np.zeros(n, dtype=np.uintp)    # the tick's pointer table
        self._len = np.empty(n, dtype=np.int32)
        self._status = np.empty(n, dtype=np.int32)
        self._call = np.empty(n, dtype=np.int32)
        self._dist = np.empty((n, self.nY), dtype=np.float32)
        self._fpt = np.empty((n, self.K), dtype=np.float64)
        self._dwell = np.empty((n, self.K), dtype=np.int64)
        self._stats = np.empty((n, 6), dtype=np.float64)
        self._ridx = np.empty((n, 3), dtype=np.int32)
        self._prob = np.empty((n, max(self.k, 1)), dtype=np.float64)
        self._pred = np.empty(n, dtype=np.int32)
        self._conf = np.empty(n, dtype=np.float64)

    def tick(self, rows: Sequence[np.ndarray], adapter_start, adapter_end, success=None, want_dist=True,
             want_fpt=False, want_dwell=False, want_stats=False, want_refine_idx=False) -> TickResult:
        """rows: one float32 1-D array per read (ragged); adapter_start/end per read (the live caller passes 0 and
        ``polya_start``, worker.py:39-44).  ``want_dist`` is ignored without references; ``want_refine_idx`` needs
        ``refine``.  Returned arrays are fresh copies."""
        return self._tick(rows, np.float32, None, None, adapter_start, adapter_end, success, want_dist, want_fpt, want_dwell,
                          want_stats, want_refine_idx)

    def tick_adc(self, adc_rows: Sequence[np.ndarray], offset, scale, adapter_start, adapter_end, success=None,
                 want_dist=True, want_fpt=False, want_dwell=False, want_stats=False, want_refine_idx=False) -> TickResult:
        """:meth:`tick` for int16 ADC rows (one 1-D int16 array per read) with each read's ``offset`` / ``scale``.  The rows
        stand for ``scale * (float32(adc) + offset)`` -- `sig_proc.calibrate_adc`, the contract of every ``*_adc`` entry
        point -- with a NaN tail behind the read's last sample: the results are, bit for bit, those of
        ``fingerprint_batch_adc`` / ``demux_batch_adc`` on a minibatch of the same reads.  (So a window that runs past its
        read's end reads NaN here, as on a minibatch; :meth:`tick`, whose rows end with the read, cuts the window there.)
        Available on any LiveDemux, next to :meth:`tick`."""
        off = np.ascontiguousarray(offset, dtype=np.float32)
        sc = np.ascontiguousarray(scale, dtype=np.float32)
        if off.shape != (len(adc_rows),) or sc.shape != (len(adc_rows),):
            raise ValueError("offset/scale must have one entry per read")
        return self._tick(adc_rows, np.int16, off, sc, adapter_start, adapter_end, success, want_dist, want_fpt, want_dwell,
                          want_stats, want_refine_idx)

    def _tick(self, rows, dtype, off, sc, adapter_start, adapter_end, success, want_dist, want_fpt, want_dwell, want_stats,
              want_refine_idx) -> TickResult:
        n = len(rows)
        self._reserve(n)
        # the pointer table: the one per-read loop of a tick on the Python side, so every step in it is the cheapest that
        # does the job (the address through the buffer protocol: `r.ctypes.data` costs three times as much)
        keep, ptrs, lens = [], [], []
        dt, adc = _DT[dtype], dtype is np.int16
        from_buffer, addressof = C.c_char.from_buffer, C.addressof
        for r in rows:
            if adc and getattr(r, "dtype", None) != dt:
                raise ValueError("tick_adc takes int16 rows (they are passed by address, never converted)")
            if type(r) is not np.ndarray or r.dtype is not dt or r.ndim != 1 or not r.flags.c_contiguous:
                r = np.ascontiguousarray(r, dtype=dt).ravel()
                keep.append(r)
            try:
                ptrs.append(addressof(from_buffer(r)))
            except (TypeError, ValueError):     # a read-only or an empty row
                ptrs.append(r.ctypes.data)
            lens.append(r.size)
        self._rows[:n] = ptrs
        self._len[:n] = lens
        a_s = np.ascontiguousarray(adapter_start, dtype=np.int32)
        a_e = np.ascontiguousarray(adapter_end, dtype=np.int32)
        if a_s.shape != (n,) or a_e.shape != (n,):
            raise ValueError("adapter_start/adapter_end must have one entry per read")
        ok = None if success is None else np.ascontiguousarray(success, dtype=np.uint8)
        if ok is not None and ok.shape != (n,):
            raise ValueError("success must have one entry per read")
        if want_refine_idx and self.refine is None:
            raise ValueError("want_refine_idx needs a LiveDemux built with refine")
        tail = self.tail != _lib.LIVE_TAIL_NONE
        want_dist = bool(want_dist) and self.nY > 0
        rows_p = _lib.addr(self._rows)
        desc = _lib.LiveInC(None if adc else rows_p, rows_p if adc else None, _lib.addr(off), _lib.addr(sc), _lib.addr(self._len),
                            n, _lib.addr(a_s), _lib.addr(a_e), _lib.addr(ok), self.tail, 0)
        bad = C.c_int64(0)

        def run(with_fpt):
            want = ((_lib.WANT_FPT if with_fpt else 0) | (_lib.WANT_DIST if want_dist else 0)
                    | (_lib.WANT_DWELL if want_dwell else 0) | (_lib.WANT_STATS if want_stats else 0)
                    | (_lib.WANT_REFINE_IDX if want_refine_idx else 0))
            out = _lib.MinibatchOutC(_lib.addr(self._status), _lib.addr(self._call), _lib.addr(self._dist) if want_dist else None,
                                     _lib.addr(self._fpt) if with_fpt else None, _lib.addr(self._dwell) if want_dwell else None,
                                     _lib.addr(self._stats) if want_stats else None, _lib.addr(self._prob) if tail else None,
                                     _lib.addr(self._pred) if tail else None, _lib.addr(self._conf) if tail else None)
            _lib.check(self.L.wdx_live_tick_ex(self.ctx.handle, C.byref(desc), C.byref(self._pc),
                                               None if self._rc is None else C.byref(self._rc), self.nY, want, C.byref(out),
                                               _lib.ptr(self._ridx) if want_refine_idx else None, C.byref(bad)))

        run(want_fpt)
        if bad.value:
            # DTW_MLP.predict's refusal (scikit-learn's, for the distances of the reads the model was shown).  Its text is
            # made from the fingerprints: the error path fetches them with a second tick, so that no good tick pays for them
            if not want_fpt:
                run(True)
            raise ValueError(self.model._nonfinite_message(self._fpt[:n][self._status[:n] == 0]))
        del keep
        status = self._status[:n].copy()
        pred = None
        if tail:
            pred = self._pred[:n].astype(np.int64)
            pred[status != 0] = -1
        return TickResult(status, self._call[:n].copy(), self._dist[:n].copy() if want_dist else None,
                          self._fpt[:n].copy() if want_fpt else None, self._prob[:n, :self.k].copy() if tail else None,
                          pred, self._conf[:n].copy() if tail else None, self._dwell[:n].copy() if want_dwell else None,
                          self._stats[:n].copy() if want_stats else None, self._ridx[:n].copy() if want_refine_idx else None)

    def close(self):
        self.ctx.close()


def demux_worker(input_queue, output_queue, live: LiveDemux, tick_seconds: float = 0.1, max_reads: int = 512) -> None:
    """Queue-to-queue mirror of ``segmentation_worker`` + ``classification_worker`` (worker.py:26-131), batched per
    tick: blocks for the first ReadObject, then takes everything else already queued (at most ``max_reads``), runs
    ONE tick and forwards each object with ``data_arr = y_prob.reshape(1, -1)``, ``is_outlier`` and
    two appended ``time_per_step`` entries (segmentation, classification: the tick's wall time split evenly -- the
    device does both in one call).  ``None`` stops the worker (and is forwarded).  Reads whose fingerprint fails
    are dropped like the reference's "no segments" branch (worker.py:75-79).  Needs ``live`` built with a model, of any
    of the three kinds.  Objects whose ``data_arr`` is int16 carry ``calibration`` = (offset, scale) and go through
    :meth:`LiveDemux.tick_adc`, float objects through :meth:`LiveDemux.tick`.  A session delivers one kind; a tick that
    holds both is refused with ``ValueError`` (the two kinds treat a window past the chunk's end differently, so neither
    can stand in for the other)."""
    if live.k == 0:
        raise ValueError("demux_worker needs a LiveDemux with a model (DTW_SVM, DTW_MLP or Fpt_Boost)")
    while True:
        first = input_queue.get()
        if first is None:
            output_queue.put(None)
            return
        batch = [first]
        stop = False
        while len(batch) < max_reads:
            try:
                nxt = input_queue.get_nowait()
            except _queue.Empty:
                break
            if nxt is None:
                stop = True
                break
            batch.append(nxt)
        t0 = time.time()
        raw = [np.asarray(o.data_arr) for o in batch]
        is_adc = [r.dtype == np.int16 for r in raw]
        a_s = np.zeros(len(batch), np.int32)
        a_e = np.array([o.polya_start for o in batch], dtype=np.int32)
        if all(is_adc):
            cal = np.array([o.calibration for o in batch], dtype=np.float32).reshape(len(batch), 2)
            r = live.tick_adc([np.ascontiguousarray(x).ravel() for x in raw], cal[:, 0], cal[:, 1], a_s, a_e, want_dist=False)
        elif any(is_adc):
            raise ValueError("demux_worker: one tick holds int16 and float ReadObjects; a session must deliver one kind")
        else:
            r = live.tick([np.asarray(x, dtype=np.float32).ravel() for x in raw], a_s, a_e, want_dist=False)
        dt = (time.time() - t0) / 2
        for i, o in enumerate(batch):
            if r.status[i] != 0:
                continue
            o.data_arr = r.prob[i].reshape(1, -1)
            o.is_outlier = bool(r.pred[i] == -1)
            o.time_per_step.append(dt)
            o.time_per_step.append(dt)
            output_queue.put(o)
        if stop:
            output_queue.put(None)
            return
