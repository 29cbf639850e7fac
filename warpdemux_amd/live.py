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

from . import _lib, _marshal
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


_DT = {np.float32: np.dtype(np.float32), np.int16: np.dtype(np.int16)}
# every array a tick can bring back: allocated once per capacity, narrowed per tick (`_marshal.out_addrs`)
_ALL = _lib.WANT_FPT | _lib.WANT_DIST | _lib.WANT_DWELL | _lib.WANT_STATS | _lib.WANT_REFINE_IDX


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

    ``long_windows``: ticks fingerprint adapter windows of up to 65 536 samples, int16 ones included (WDX_OPT_LONG_WINDOWS;
    refined ticks: WDX_OPT_LONG_REFINE_WINDOWS).

    ``wide_dtw``: effective windows 33 .. L (``window=None`` on fingerprints of 33 .. 256 events) run on the wide-window DTW
    kernel instead of the scratch rows (WDX_OPT_WIDE_DTW); same results.

    Every check of the arguments happens before a context is created and raises ``ValueError``."""

    def __init__(self, refs=None, window=None, penalty=None, params: Optional[SegParams] = None, *, model=None,
                 refine: Optional[RefineParams] = None, adc: bool = False, device: int = 0, max_reads: int = 512,
                 max_samples: int = 10000, long_windows: bool = False, wide_dtw: bool = False):
        wide_dtw = _marshal.wide_dtw_option(wide_dtw, "LiveDemux")
        optimal = _marshal.refine_options(refine, long_windows, "LiveDemux")
        d = _marshal.deployment(
            refs, window, penalty, params, model, refine, who="LiveDemux", models=("DTW_SVM", "DTW_MLP", "Fpt_Boost"),
            bare_refine=False, refine_dtw=False,
            nothing_to_serve="refs may only be None with an Fpt_Boost model (its tail needs no references)")
        self.tail, self.model, self.refine, self.params, self.nY, self.K, self.k = (d.kind, model, refine, d.params, d.nY, d.K,
                                                                                   d.n_classes)
        self._pc = self.params.to_c()
        self._rc = None if refine is None else refine.to_c()

        self.L = _lib.load()
        self.ctx = _lib.Context(device)      # this object's own context = own stream + staging buffers
        if long_windows:
            self.ctx.set_long_windows()
        if optimal:   # refine.optimal_cpts: refined ticks cut the barcode tail at its optimal change-points
            self.ctx.set_option(_lib.OPT_REFINE_OPTIMAL_CPTS, 1)
        if wide_dtw:
            self.ctx.set_option(_lib.OPT_WIDE_DTW, 1)
        if self.nY:
            _marshal.set_refs(self.ctx, d.refs, d.window, d.penalty)
        if model is not None:
            _marshal.set_model(self.ctx, model)
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
        self._out = _marshal.outputs(n, self.K, self.nY, self.k, _ALL | (_marshal.WANT_TAIL if self.k else 0))

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
        n = len(adc_rows)
        off, sc = _marshal.per_read(n, np.float32, "offset/scale", offset), _marshal.per_read(n, np.float32, "offset/scale", scale)
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
        a_s, a_e, ok = _marshal.windows(n, adapter_start, adapter_end, success)
        if want_refine_idx and self.refine is None:
            raise ValueError("want_refine_idx needs a LiveDemux built with refine")
        tail = _marshal.WANT_TAIL if self.tail != _lib.LIVE_TAIL_NONE else 0
        want_dist = bool(want_dist) and self.nY > 0
        rows_p = _lib.addr(self._rows)
        desc = _lib.LiveInC(None if adc else rows_p, rows_p if adc else None, _lib.addr(off), _lib.addr(sc), _lib.addr(self._len),
                            n, _lib.addr(a_s), _lib.addr(a_e), _lib.addr(ok), self.tail, 0)
        bad = C.c_int64(0)
        o = self._out

        def run(with_fpt):
            want = ((_lib.WANT_FPT if with_fpt else 0) | (_lib.WANT_DIST if want_dist else 0)
                    | (_lib.WANT_DWELL if want_dwell else 0) | (_lib.WANT_STATS if want_stats else 0)
                    | (_lib.WANT_REFINE_IDX if want_refine_idx else 0))
            out = _marshal.out_c(o, want | tail)     # (the tail is named in `desc`, not in the bits the library reads)
            _lib.check(self.L.wdx_live_tick_ex(self.ctx.handle, C.byref(desc), C.byref(self._pc),
                                               None if self._rc is None else C.byref(self._rc), self.nY, want, C.byref(out),
                                               _lib.ptr(o["refine_idx"]) if want_refine_idx else None, C.byref(bad)))

        run(want_fpt)
        if bad.value:
            # DTW_MLP.predict's refusal (scikit-learn's, for the distances of the reads the model was shown).  Its text is
            # made from the fingerprints: the error path fetches them with a second tick, so that no good tick pays for them
            if not want_fpt:
                run(True)
            raise ValueError(self.model._nonfinite_message(o["fpt"][:n][o["status"][:n] == 0]))
        del keep
        status = o["status"][:n].copy()
        pred = None
        if tail:
            pred = o["pred"][:n].astype(np.int64)
            pred[status != 0] = -1

        def got(name, wanted):
            return o[name][:n].copy() if wanted else None

        return TickResult(status, got("call", True), got("dist", want_dist), got("fpt", want_fpt), got("prob", tail), pred,
                          got("conf", tail), got("dwell", want_dwell), got("stats", want_stats), got("refine_idx", want_refine_idx))

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
