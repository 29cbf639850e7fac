"""Pipelined minibatches for the reference's worker loop (file_proc.py:380-454, 1197-1243).

A WarpDemuX worker alternates "fill minibatch k+1" (pod5 reads -> one (1000, sig_preload_size) float32 array,
file_proc.py:244-260) with "process minibatch k".  `MinibatchPipeline` gives that loop two things the plain
`sig_proc.demux_batch` call cannot:

* page-locked minibatch buffers (`pinned_empty`) the worker fills in place of ``np.full(...)`` -- the GPU reads them
  by DMA at the bus rate instead of through the runtime's pageable staging;
* `submit(slot, ...)` / `wait(slot)` (C ABI: wdx_demux_submit / wdx_demux_wait): two minibatches in flight on two
  streams of one context, so the copy-in of k+1 overlaps the kernels and the copy-out of k while the worker's own
  thread fills the next buffer.

Results are bit-identical to `demux_batch` (same kernels).  INTEGRATION.md shows the four-line change in
``file_proc``'s loop.

``MinibatchPipeline(..., refine=RefineParams(...))`` runs the consensus-refinement branch of the tRNA models on the same
slots (wdx_demux_submit_refine / wdx_demux_wait_refine): `wait` then returns a `RefineMinibatch` -- the arrays of
`sig_proc.fingerprint_refine_batch`, bit for bit, plus call / dist when there are references; ``refs=None`` is a
fingerprint-only pipeline.

``MinibatchPipeline(refs=None, ..., model=Fpt_Boost, refine=...)`` is the tRNA flow from one pass: the model
(`models.Fpt_Boost`, the class of both tRNA models) is resident on the device and every minibatch asks for WDX_WANT_BOOST,
so `wait` returns a `BoostMinibatch` -- the ReadResult arrays and ``Fpt_Boost.predict`` of the fingerprints (prob / pred /
conf; failed reads -1 / NaN).  It needs no references, with or without ``refine``.
"""
from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from .sig_proc import DemuxBatch, FingerprintBatch, RefineParams, SegParams, adc_minibatch


def pinned_empty(shape, dtype=np.float32, device: Optional[int] = None) -> np.ndarray:
    """Uninitialised NumPy array in page-locked host memory (wdx_host_alloc); freed with the array.  ``device``: the
    GPU whose context will read it (wdx_host_alloc_on: no stray HIP context on device 0 in a multi-GPU worker)."""
    dtype = np.dtype(dtype)
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(v) for v in shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    L = _lib.load()
    p = C.c_void_p()
    if device is None:
        _lib.check(L.wdx_host_alloc(C.c_size_t(nbytes), C.byref(p)))
    else:
        _lib.check(L.wdx_host_alloc_on(int(device), C.c_size_t(nbytes), C.byref(p)))
    buf = (C.c_char * max(nbytes, 1)).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)
    weakref.finalize(buf, L.wdx_host_free, C.c_void_p(p.value))   # the ctypes block lives as long as any view of it
    return arr


def pinned_full(shape, fill_value, dtype=np.float32, device: Optional[int] = None) -> np.ndarray:
    """``np.full`` in page-locked memory: the drop-in for file_proc.py:244 (``np.full((n, m), np.nan, float32)``)."""
    a = pinned_empty(shape, dtype, device)
    a.fill(fill_value)
    return a


MAX_SLOTS = 8   # WDX_MAX_SLOTS (include/wdx.h)


def register_host(arr: np.ndarray):
    """Page-lock memory the caller owns (wdx_host_register) -- e.g. a multiprocessing.shared_memory block that producer
    processes fill while ONE feeder process owns the context.  Returns a finalizer-like callable that unregisters."""
    L = _lib.load()
    p = C.c_void_p(arr.ctypes.data)
    _lib.check(L.wdx_host_register(p, C.c_size_t(arr.nbytes)))
    return lambda: L.wdx_host_unregister(p)


@dataclass
class RefineMinibatch:
    """What `MinibatchPipeline.wait` returns for a refine pipeline: `fingerprints` (with ``refine_idx``) is
    `sig_proc.fingerprint_refine_batch`'s result; call is -1 everywhere and dist None without references."""

    fingerprints: FingerprintBatch
    call: np.ndarray
    dist: Optional[np.ndarray]

    @property
    def status(self) -> np.ndarray:
        return self.fingerprints.status


@dataclass
class BoostMinibatch:
    """What `MinibatchPipeline.wait` returns for a pipeline with a boost model: `fingerprints` is
    `sig_proc.fingerprint_batch`'s (with ``refine``: `fingerprint_refine_batch`'s) result, prob / pred / conf what
    ``Fpt_Boost.predict_raw`` gives on the fingerprints -- pred int64 labels, -1 for rejected and for failed reads, whose
    prob / conf are NaN; call is -1 everywhere and dist None without references."""

    fingerprints: FingerprintBatch
    call: np.ndarray
    dist: Optional[np.ndarray]
    prob: np.ndarray
    pred: np.ndarray
    conf: np.ndarray

    @property
    def status(self) -> np.ndarray:
        return self.fingerprints.status


class MinibatchPipeline:
    """Minibatches in flight against one resident reference set (model._X): two slots for a worker's own loop, up to
    MAX_SLOTS for a feeder process that serves many producers.  ``refine``: every minibatch takes the
    consensus-refinement branch (K = ``refine.barcode_keep_events``); then ``refs`` may be None (fingerprints only).
    ``model``: a `models.Fpt_Boost` kept resident on the device; every minibatch brings its prediction back
    (`BoostMinibatch`), ``refs`` may be None, and K must equal ``model.n_features``."""

    N_SLOTS = 2

    def __init__(self, refs=None, window=None, penalty=None, params: Optional[SegParams] = None, device: int = 0,
                 n_slots: int = 2, refine: Optional[RefineParams] = None, model=None):
        if not 1 <= int(n_slots) <= MAX_SLOTS:
            raise ValueError(f"n_slots must be in [1, {MAX_SLOTS}]")
        self.N_SLOTS = int(n_slots)
        self.refine = refine
        self.model = model
        if refs is None:
            if refine is None and model is None:
                raise ValueError("refs is required (only a refine pipeline or one with a boost model can do without)")
            k0 = int(refine.barcode_keep_events) if refine is not None else (
                int(params.barcode_num_events) if params is not None else int(model.n_features))
            refs = np.zeros((0, k0), dtype=np.float64)
        refs = np.ascontiguousarray(refs, dtype=np.float64)
        if refs.ndim != 2:
            raise ValueError("refs must be (nY, L)")
        K = int(refine.barcode_keep_events) if refine is not None else int(refs.shape[1])
        self.params = params or SegParams(barcode_num_events=K)
        if K != refs.shape[1] or (refine is None and self.params.barcode_num_events != K):
            raise ValueError("barcode_num_events must equal the reference length")
        if model is not None and K != int(model.n_features):
            raise ValueError(f"the fingerprints have {K} events but the boost model takes {int(model.n_features)} features")
        self.nY, self.K = (int(v) for v in refs.shape)
        self.L = _lib.load()
        self.ctx = _lib.Context(device)
        if self.nY:
            _lib.check(self.L.wdx_set_refs(self.ctx.handle, _lib.ptr(refs), self.nY, self.K,
                                           int(window) if window else 0, float(penalty) if penalty else 0.0))
        if model is not None:
            m = model.to_c()
            _lib.check(self.L.wdx_boost_set_model(self.ctx.handle, C.byref(m)))
        self._pc = self.params.to_c()
        self._rc = refine.to_c() if refine is not None else None
        self._held = [None] * self.N_SLOTS     # the submitted arrays must outlive the copy-in

    def submit(self, slot: int, signals, adapter_start, adapter_end, success=None, want_dist=True, want_fpt=False):
        """Enqueue one minibatch on `slot` (0 or 1) and return.  `signals` must not be modified before `wait(slot)`."""
        sig = np.asarray(signals)
        if sig.ndim != 2:
            raise ValueError("signals must be a 2-D (n_reads, stride) array")
        sig = np.ascontiguousarray(sig, dtype=np.float32)
        n, stride = sig.shape
        a_s = np.ascontiguousarray(adapter_start, dtype=np.int32)
        a_e = np.ascontiguousarray(adapter_end, dtype=np.int32)
        if a_s.shape != (n,) or a_e.shape != (n,):
            raise ValueError("adapter_start/adapter_end must have one entry per read")
        ok = None if success is None else np.ascontiguousarray(success, dtype=np.uint8)
        if not 0 <= int(slot) < self.N_SLOTS:
            raise ValueError(f"slot must be in [0, {self.N_SLOTS})")
        if self.refine is not None or self.model is not None:
            desc = _lib.MinibatchInC(_lib.addr(sig), n, stride, None, None, _lib.addr(a_s), _lib.addr(a_e), _lib.addr(ok))
            want_dist = bool(want_dist) and self.nY > 0
            self._submit_all(slot, desc, None, want_dist)
            self._held[slot] = (sig, a_s, a_e, ok, n, want_dist, True)
            return
        _lib.check(self.L.wdx_demux_submit(self.ctx.handle, int(slot), _lib.ptr(sig), n, stride, _lib.ptr(a_s),
                                           _lib.ptr(a_e), _lib.ptr(ok), C.byref(self._pc), self.nY, int(want_fpt),
                                           int(want_dist)))
        self._held[slot] = (sig, a_s, a_e, ok, n, bool(want_dist), bool(want_fpt))

    def _submit_all(self, slot: int, desc, desc_adc, want_dist: bool):
        """a refine minibatch, and one of a pipeline with a boost model, always brings the ReadResult arrays back -- with a
        model, its prediction too (WDX_WANT_BOOST)"""
        want = (_lib.WANT_FPT | _lib.WANT_DWELL | _lib.WANT_STATS | (_lib.WANT_DIST if want_dist else 0) |
                (_lib.WANT_REFINE_IDX if self.refine is not None else 0) | (_lib.WANT_BOOST if self.model is not None else 0))
        f = None if desc is None else C.byref(desc)
        a = None if desc_adc is None else C.byref(desc_adc)
        if self.refine is not None:
            rc = self.L.wdx_demux_submit_refine(self.ctx.handle, int(slot), f, a, C.byref(self._pc), C.byref(self._rc), self.nY,
                                                want)
        elif desc_adc is not None:
            rc = self.L.wdx_demux_submit_adc(self.ctx.handle, int(slot), a, C.byref(self._pc), self.nY, want)
        else:
            rc = self.L.wdx_demux_submit_ex(self.ctx.handle, int(slot), f, C.byref(self._pc), self.nY, want)
        _lib.check(rc)

    def submit_adc(self, slot: int, adc, row_len, offset, scale, adapter_start, adapter_end, success=None, want_dist=True,
                   want_fpt=False, row_off=None, row_win=None):
        """`submit` for an int16 ADC minibatch (wdx_demux_submit_adc): ``adc`` (n_reads, stride) int16 -- fill a
        ``pinned_empty(shape, np.int16)`` buffer and only the adapter windows cross the bus, 2 bytes per sample --
        with ``row_len`` / ``offset`` / ``scale`` per read; the device calibrates (`sig_proc.calibrate_adc` states the
        formula).  With ``row_off`` the rows are packed by the caller (`sig_proc.adc_minibatch`).  `wait(slot)` returns
        what `submit` + `wait` return on the calibrated rows, bit for bit.  Nothing passed here may be modified before
        `wait(slot)`."""
        if not 0 <= int(slot) < self.N_SLOTS:
            raise ValueError(f"slot must be in [0, {self.N_SLOTS})")
        desc, n, kept = adc_minibatch(adc, row_len, offset, scale, adapter_start, adapter_end, success, row_off, row_win)
        if self.refine is not None or self.model is not None:
            want_dist = bool(want_dist) and self.nY > 0
            self._submit_all(slot, None, desc, want_dist)
            self._held[slot] = (kept, None, None, None, n, want_dist, True)
            return
        want = (_lib.WANT_FPT if want_fpt else 0) | (_lib.WANT_DIST if want_dist else 0)
        _lib.check(self.L.wdx_demux_submit_adc(self.ctx.handle, int(slot), C.byref(desc), C.byref(self._pc), self.nY, want))
        self._held[slot] = (kept, None, None, None, n, bool(want_dist), bool(want_fpt))

    def wait(self, slot: int):
        """`DemuxBatch` of the minibatch on `slot`; a refine pipeline returns a `RefineMinibatch`, one with a boost model a
        `BoostMinibatch`."""
        held = self._held[slot] if 0 <= int(slot) < self.N_SLOTS else None
        if held is None:
            raise ValueError(f"nothing was submitted on slot {slot}")
        n, want_dist, want_fpt = held[4:]
        if self.refine is not None or self.model is not None:
            return self._wait_all(slot, n, want_dist)
        dist = np.empty((n, self.nY), dtype=np.float32) if want_dist else None
        fpt = np.empty((n, self.K), dtype=np.float64) if want_fpt else None
        call = np.empty(n, dtype=np.int32)
        status = np.empty(n, dtype=np.int32)
        rc = self.L.wdx_demux_wait(self.ctx.handle, int(slot), _lib.ptr(fpt), _lib.ptr(dist), _lib.ptr(call),
                                   _lib.ptr(status))
        # WDX_ERR_INVALID (an argument error, or another thread already waiting on this slot) leaves the minibatch IN
        # FLIGHT in the slot (wdx.h): the copy-in may still be reading the arrays, so they stay referenced and the
        # caller can wait again.  Success and a HIP error both free the slot on the C side.
        if rc != _lib.WDX_ERR_INVALID:
            self._held[slot] = None
        _lib.check(rc)
        return DemuxBatch(status, call, dist, fpt)

    def _wait_all(self, slot: int, n: int, want_dist: bool):
        fb = FingerprintBatch(np.empty((n, self.K), dtype=np.float64), np.empty((n, self.K), dtype=np.int64),
                              np.empty((n, 6), dtype=np.float64), np.empty(n, dtype=np.int32),
                              np.empty((n, 3), dtype=np.int32) if self.refine is not None else None)
        call = np.empty(n, dtype=np.int32)
        dist = np.empty((n, self.nY), dtype=np.float32) if want_dist else None
        prob = pred = conf = None
        if self.model is not None:
            prob, pred, conf = np.empty((n, int(self.model.k))), np.empty(n, dtype=np.int32), np.empty(n)
        out = _lib.MinibatchOutC(_lib.addr(fb.status), _lib.addr(call), _lib.addr(dist), _lib.addr(fb.fpt), _lib.addr(fb.dwell),
                                 _lib.addr(fb.stats), _lib.addr(prob), _lib.addr(pred), _lib.addr(conf))
        rc = self.L.wdx_demux_wait_refine(self.ctx.handle, int(slot), C.byref(out), _lib.ptr(fb.refine_idx))
        if rc != _lib.WDX_ERR_INVALID:   # (as in `wait`: an argument error leaves the minibatch in flight)
            self._held[slot] = None
        _lib.check(rc)
        if self.model is not None:
            return BoostMinibatch(fb, call, dist, prob, pred.astype(np.int64), conf)
        return RefineMinibatch(fb, call, dist)

    def run(self, minibatches):
        """Drive an iterable of (signals, adapter_start, adapter_end[, success]) through both slots; yields one
        DemuxBatch per minibatch, in order.  The iterable is advanced (= the caller's fill runs) while the previous
        minibatch is in flight.  A tuple whose first entry is an int16 array is an ADC minibatch: (adc, row_len, offset,
        scale, adapter_start, adapter_end[, success, ...]), the arguments of `submit_adc`.

        Order per minibatch k: wait(k - 2), THEN next(iterable), then submit(k) -- so a generator that refills two
        rotating page-locked buffers never writes into a buffer whose submit has not been waited
        for (submit()'s contract, wdx.h: inputs stay untouched until the matching wait); minibatch k - 1 is still in
        flight while the generator fills buffer k."""
        it = iter(minibatches)
        pending = []
        k = 0
        while True:
            slot = k % self.N_SLOTS
            if len(pending) == self.N_SLOTS:   # the slot (and the caller's buffer) about to be reused
                yield self.wait(pending.pop(0))
            try:
                mb = next(it)
            except StopIteration:
                break
            if isinstance(mb[0], np.ndarray) and mb[0].dtype == np.int16:
                self.submit_adc(slot, *mb)
            else:
                self.submit(slot, *mb)
            pending.append(slot)
            k += 1
        for slot in pending:
            yield self.wait(slot)

    def close(self):
        self.ctx.close()
