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

from . import _lib, _marshal
from .sig_proc import DemuxBatch, FingerprintBatch, RefineParams, SegParams, adc_minibatch, fingerprints


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
    (`BoostMinibatch`), ``refs`` may be None, and K must equal ``model.n_features``.
    ``long_windows``: minibatches fingerprint adapter windows of up to 65 536 samples (WDX_OPT_LONG_WINDOWS; with ``refine``:
    WDX_OPT_LONG_REFINE_WINDOWS).
    ``wide_dtw``: effective windows 33 .. L (``window=None`` on fingerprints of 33 .. 256 events) run on the wide-window DTW
    kernel instead of the scratch rows (WDX_OPT_WIDE_DTW); same results."""

    N_SLOTS = 2

    def __init__(self, refs=None, window=None, penalty=None, params: Optional[SegParams] = None, device: int = 0,
                 n_slots: int = 2, refine: Optional[RefineParams] = None, model=None, long_windows: bool = False,
                 wide_dtw: bool = False):
        wide_dtw = _marshal.wide_dtw_option(wide_dtw, "MinibatchPipeline")
        if not 1 <= int(n_slots) <= MAX_SLOTS:
            raise ValueError(f"n_slots must be in [1, {MAX_SLOTS}]")
        self.N_SLOTS = int(n_slots)
        optimal = _marshal.refine_options(refine, long_windows, "MinibatchPipeline")
        d = _marshal.deployment(
            refs, window, penalty, params, model, refine, who="MinibatchPipeline", models=("Fpt_Boost",), bare_refine=True,
            refine_dtw=True,
            nothing_to_serve="refs is required (only a refine pipeline or one with a boost model can do without)")
        self.refine, self.model, self.params, self.nY, self.K, self._n_classes = refine, model, d.params, d.nY, d.K, d.n_classes
        self.L = _lib.load()
        self.ctx = _lib.Context(device)
        if long_windows:   # (every slot copies the context's options at its submit; 12 MB per slot that meets a long window)
            self.ctx.set_long_windows()
        if optimal:   # refine.optimal_cpts: WDX_OPT_REFINE_OPTIMAL_CPTS (the slots copy it like every option)
            self.ctx.set_option(_lib.OPT_REFINE_OPTIMAL_CPTS, 1)
        if wide_dtw:
            self.ctx.set_option(_lib.OPT_WIDE_DTW, 1)
        if self.nY:
            _marshal.set_refs(self.ctx, d.refs, d.window, d.penalty)
        if model is not None:
            _marshal.set_model(self.ctx, model)
        self._pc = self.params.to_c()
        self._rc = refine.to_c() if refine is not None else None
        # a refine minibatch, and one of a pipeline with a boost model, always brings the ReadResult arrays back -- with a
        # model, its prediction too (WDX_WANT_BOOST) -- through the wdx_minibatch_in / _out entry points
        self._all = 0
        if refine is not None or model is not None:
            self._all = (_lib.WANT_FPT | _lib.WANT_DWELL | _lib.WANT_STATS | (_lib.WANT_REFINE_IDX if refine is not None else 0) |
                         (_lib.WANT_BOOST if model is not None else 0))
        self._held = [None] * self.N_SLOTS     # (the submitted arrays, which must outlive the copy-in; n_reads; want)

    def _want(self, slot: int, want_dist, want_fpt) -> int:
        if not 0 <= int(slot) < self.N_SLOTS:
            raise ValueError(f"slot must be in [0, {self.N_SLOTS})")
        if self._all:
            return self._all | (_lib.WANT_DIST if want_dist and self.nY > 0 else 0)
        return (_lib.WANT_FPT if want_fpt else 0) | (_lib.WANT_DIST if want_dist else 0)

    def submit(self, slot: int, signals, adapter_start, adapter_end, success=None, want_dist=True, want_fpt=False):
        """Enqueue one minibatch on `slot` (0 or 1) and return.  `signals` must not be modified before `wait(slot)`."""
        sig, a_s, a_e, ok, n, stride = kept = _marshal.minibatch(signals, adapter_start, adapter_end, success)
        want = self._want(slot, want_dist, want_fpt)
        if self._all:
            desc = _lib.MinibatchInC(_lib.addr(sig), n, stride, None, None, _lib.addr(a_s), _lib.addr(a_e), _lib.addr(ok))
            self._submit_all(slot, desc, None, want)
        else:
            _lib.check(self.L.wdx_demux_submit(self.ctx.handle, int(slot), _lib.ptr(sig), n, stride, _lib.ptr(a_s),
                                               _lib.ptr(a_e), _lib.ptr(ok), C.byref(self._pc), self.nY, int(bool(want_fpt)),
                                               int(bool(want_dist))))
        self._held[slot] = (kept, n, want)

    def _submit_all(self, slot: int, desc, desc_adc, want: int):
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
        want = self._want(slot, want_dist, want_fpt)
        desc, n, kept = adc_minibatch(adc, row_len, offset, scale, adapter_start, adapter_end, success, row_off, row_win)
        self._submit_all(slot, None, desc, want)
        self._held[slot] = (kept, n, want)

    def wait(self, slot: int):
        """`DemuxBatch` of the minibatch on `slot`; a refine pipeline returns a `RefineMinibatch`, one with a boost model a
        `BoostMinibatch`."""
        held = self._held[slot] if 0 <= int(slot) < self.N_SLOTS else None
        if held is None:
            raise ValueError(f"nothing was submitted on slot {slot}")
        _, n, want = held
        o = _marshal.outputs(n, self.K, self.nY, self._n_classes, want)
        if self._all:
            out = _marshal.out_c(o)
            rc = self.L.wdx_demux_wait_refine(self.ctx.handle, int(slot), C.byref(out), _lib.ptr(o["refine_idx"]))
        else:
            rc = self.L.wdx_demux_wait(self.ctx.handle, int(slot), _lib.ptr(o["fpt"]), _lib.ptr(o["dist"]), _lib.ptr(o["call"]),
                                       _lib.ptr(o["status"]))
        # WDX_ERR_INVALID (an argument error, or another thread already waiting on this slot) leaves the minibatch IN
        # FLIGHT in the slot (wdx.h): the copy-in may still be reading the arrays, so they stay referenced and the
        # caller can wait again.  Success and a HIP error both free the slot on the C side.
        if rc != _lib.WDX_ERR_INVALID:
            self._held[slot] = None
        _lib.check(rc)
        if self.model is not None:
            return BoostMinibatch(fingerprints(o), o["call"], o["dist"], o["prob"], o["pred"].astype(np.int64), o["conf"])
        if self.refine is not None:
            return RefineMinibatch(fingerprints(o), o["call"], o["dist"])
        return DemuxBatch(o["status"], o["call"], o["dist"], o["fpt"])

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
