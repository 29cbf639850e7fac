"""Device-resident fused pipeline: raw adapter rows -> fingerprint -> DTW -> barcode call.

PyTorch is used only as plumbing (HBM allocations, the current HIP stream); all arithmetic is in
libwdx_hip.so through the ``*_dev`` entry points of include/wdx.h.  This is the path bench.py
times and the one a long-running WarpDemuX worker would keep open per GPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib, _marshal, _medoids, _nearest, synth
from .sig_proc import DetectParams, SegParams


def _torch():
    import torch

    return torch


def _dp(t):
    """device pointer of a torch tensor (None -> NULL)"""
    return None if t is None else C.c_void_p(t.data_ptr())


@dataclass
class AdcShard:
    """Raw int16 ADC reads that stay int16 in HBM (wdx_adc_dev_in, include/wdx.h), accepted wherever a `DemuxEngine` method
    takes ``sig``: read r stands for the float32 row ``scale[r] * (float32(adc) + offset[r])`` -- float32 add, then float32
    multiply, `sig_proc.calibrate_adc` -- with a NaN tail behind its ``row_len[r]`` samples, and every method returns, bit
    for bit, what it returns on those float32 rows.  Only that formula: a reader that calibrates otherwise must not use it.

    ``adc``: int16 device tensor -- (n, stride) rows (``stride`` defaults to its second dimension), or packed reads with
    int64 ``offsets`` of n + 1 entries, each a multiple of 8; ``row_len`` int32 (n,), ``offset`` / ``scale`` float32 (n,);
    ``row_win`` (packed only, optional) int32 (n,): samples of the float32 row read r stands for, the NaN tail included.
    ``a_start`` / ``a_end`` of the call are relative to the row.  The method's own ``offsets=`` / ``stride=`` are not used."""
    adc: "object"
    row_len: "object"
    offset: "object"
    scale: "object"
    offsets: Optional["object"] = None
    stride: int = 0
    row_win: Optional["object"] = None

    def __post_init__(self):
        torch = _torch()
        want = [("adc", self.adc, torch.int16), ("row_len", self.row_len, torch.int32), ("offset", self.offset, torch.float32),
                ("scale", self.scale, torch.float32), ("offsets", self.offsets, torch.int64), ("row_win", self.row_win, torch.int32)]
        for name, t, dt in want:
            if t is None:
                continue
            if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"AdcShard.{name} must be a contiguous {dt} device tensor")
        n = int(self.row_len.shape[0])
        if tuple(self.offset.shape) != (n,) or tuple(self.scale.shape) != (n,):
            raise ValueError("AdcShard: row_len, offset and scale hold one entry per read")
        if self.offsets is not None:
            if tuple(self.offsets.shape) != (n + 1,):
                raise ValueError("AdcShard.offsets holds n + 1 entries")
        else:
            if self.row_win is not None:
                raise ValueError("AdcShard.row_win describes packed reads: give `offsets`")
            if not self.stride:
                if self.adc.dim() != 2:
                    raise ValueError("packed reads need `offsets`, strided ones a 2-D `adc` or `stride`")
                self.stride = int(self.adc.shape[1])
        if self.row_win is not None and tuple(self.row_win.shape) != (n,):
            raise ValueError("AdcShard.row_win holds one entry per read")
        # the kernel reads adc through these numbers: what the shapes can show is checked here, on the host
        if self.offsets is None:
            if self.stride < 0 or (self.adc.dim() == 2 and (int(self.adc.shape[0]) != n or int(self.adc.shape[1]) != self.stride)):
                raise ValueError(f"AdcShard: a 2-D adc holds one row of `stride` samples per read ({n} x {self.stride}), "
                                 f"not {tuple(self.adc.shape)}")
            if int(self.adc.numel()) < n * int(self.stride):
                raise ValueError(f"AdcShard.adc holds {int(self.adc.numel())} samples, {n} rows of {self.stride} need more")
        elif n and int(self.adc.numel()) < int(self.offsets[-1].item()):
            raise ValueError(f"AdcShard.adc holds {int(self.adc.numel())} samples, its last offset is "
                             f"{int(self.offsets[-1].item())}")

    @property
    def n_reads(self):
        return int(self.row_len.shape[0])

    def to_c(self):
        return _lib.AdcDevInC(adc=self.adc.data_ptr(), row_off=None if self.offsets is None else self.offsets.data_ptr(),
                              stride=int(self.stride), row_len=self.row_len.data_ptr(), offset=self.offset.data_ptr(),
                              scale=self.scale.data_ptr(), row_win=None if self.row_win is None else self.row_win.data_ptr())

    def nbytes(self):
        """device bytes the shard's tensors hold"""
        ts = [self.adc, self.row_len, self.offset, self.scale, self.offsets, self.row_win]
        return sum(int(t.numel()) * t.element_size() for t in ts if t is not None)


@dataclass
class DemuxResult:
    dist: "object"      # torch float32 (n, nY)
    call: "object"      # torch int32 (n,)  argmin column, -1 for failed reads
    status: "object"    # torch int32 (n,)  WDX_READ_*
    counts: "object"    # torch int64 (nY+1,) accumulated call histogram (slot nY = failed)
    fpt: Optional["object"] = None   # torch float64 (n, K) when requested


@dataclass
class DetectResult:
    a_start: "object"   # torch int32 (n,)  adapter start, -1 where none was found
    a_end: "object"     # torch int32 (n,)  adapter end, -1 unless the read succeeded
    ok: "object"        # torch uint8 (n,)
    code: "object"      # torch int32 (n,)  WDX_DETECT_*
    info: Optional["object"] = None   # torch int32 (n, 4) when requested: {n, c, P[e] - P[s], P[e + polya_win] - P[e]}
    gain: Optional["object"] = None   # torch float64 (n,) when requested: g(c)


@dataclass
class NearestResult:
    call: "object"      # torch int32 (n,)   label of the nearest reference, -1 when rejected or failed
    best: "object"      # torch float32 (n, 2)  d1 = distance to the nearest reference, d2 = to the nearest of another label
    status: "object"    # torch int32 (n,)  WDX_READ_* (`nearest`: the caller's tensor, or None)
    counts: "object"    # torch int64 (G+1,) accumulated per-label histogram (slot G = every call of -1)
    dist: Optional["object"] = None   # torch float32 (n, nY) when requested
    fpt: Optional["object"] = None    # torch float64 (n, K) when requested (`demux_nearest`)


@dataclass
class MedoidResult:
    index: "object"        # torch int64 (G,)  row of each label's medoid, -1 for a label without a member
    refs: "object"         # torch float64 (G, L)  X[index] bit for bit (a NaN row without a member): goes straight into `set_refs`
    count: "object"        # torch int64 (G,)  members of each label
    medoid_cost: "object"  # torch float64 (G,)  cost[index], NaN without a member
    cost: Optional["object"] = None   # torch float64 (n,) when requested: every member's summed distance, NaN for the others


@dataclass
class DbaResult:
    centres: "object"      # torch float64 (G, L)  the new centres (a NaN row for an idle label): goes straight into `set_refs`
    count: "object"        # torch int64 (G,)  members of each label (0 for an idle label)
    inertia: "object"      # torch float64 (G,)  summed cost of the centres the step received, NaN for an idle label
    cost: Optional["object"] = None   # torch float64 (n,) when requested: D[L][L] of every member, not rooted; NaN for the others
    runs: Optional["object"] = None   # torch int32 (n, L, 2) when requested: rows lo .. hi matched to each centre point, -1 for the others


@dataclass
class LooResult:
    nn: "object"           # torch int32 (n, 2)  {own, other}: the nearest other row of the row's label, the nearest row of another label; -1 without one
    best: "object"         # torch float32 (n, 2)  the distances to them (+inf without a candidate, NaN for a non-member)


@dataclass
class SvmSolveResult:
    alpha: "object"        # torch float64 (len(rows),)  alpha of every entry of the row list
    rho: "object"          # torch float64 (n_problems,)
    n_iter: "object"       # torch int64 (n_problems,)
    state: "object"        # torch int32 (n_problems,)  0 converged, 1 iteration cap, 2 stopped (non-finite gradient / no second index)
    dec: "object"          # torch float64 (len(eval_rows),)  decision values of the evaluation rows


@dataclass
class SvmCvResult:
    prob: "object"         # torch float64 (m, k)  out-of-fold probabilities, member-row order (NaN: a problem of the row's fold stopped)
    pred_idx: "object"     # torch int32 (m,)  np.argmax of them (the class INDEX; -1 with NaN probabilities)
    conf: "object"         # torch float64 (m,)  top1 - top2
    fold_of_row: "object"  # numpy int32 (m,)  the fold that holds the row out
    folds: list            # per fold (n_support, support, dual_coef, rho, probA, probB); support numbers the rows of train[f]
    train: list            # per fold T_f: the member rows it was fitted on, ascending
    held: list             # per fold H_f
    fit_info: dict         # per problem of the one launch: pair, fold (-1: a full problem), part (fold, or cv: the full data), rows, n_iter, state
    full: "object"         # with_full: the full data's (n_support, support, dual_coef, rho, probA, probB), else None
    plan: "object"         # the `_svm_cv.CvPlan`
    solution: "object"     # the `_svm_fit.Solution` (host arrays) of the one launch


class DemuxEngine:
    """One engine per process per GPU.  ``refs``: (nY, L) float64 reference fingerprints
    (model._X in the reference, models/dtw_base.py:20).  ``wide_dtw``: effective windows 33 .. L (``window=None`` on
    fingerprints of 33 .. 256 events) run on the wide-window DTW kernel (WDX_OPT_WIDE_DTW); without it `demux` and its kin
    refuse such references (``NotImplementedError``: the fused entries need window <= 32)."""

    def __init__(self, refs: np.ndarray, window: Optional[int] = 15, penalty: Optional[float] = 0.1,
                 params: Optional[SegParams] = None, device: int = 0, long_windows: bool = False,
                 wide_dtw: bool = False):
        wide_dtw = _marshal.wide_dtw_option(wide_dtw, "DemuxEngine")
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.WdxError("DemuxEngine needs a visible MI355X (torch.cuda.is_available() is False)")
        self.torch = torch
        self.device = int(device)
        self.tdev = torch.device("cuda", self.device)
        self.ctx = _lib.Context(self.device)
        if long_windows:   # adapter windows of up to 65 536 samples: WDX_OPT_LONG_WINDOWS (the plain entries) and
            self.ctx.set_long_windows()   # WDX_OPT_LONG_REFINE_WINDOWS (the refining ones)
        if wide_dtw:   # windows beyond 32 (``window=None`` on long fingerprints) on the wide-window kernel: WDX_OPT_WIDE_DTW
            self.ctx.set_option(_lib.OPT_WIDE_DTW, 1)
        self.L = _lib.load()
        self.params = params or SegParams(barcode_num_events=int(np.asarray(refs).shape[1]))
        self.set_refs(refs, window, penalty)
        self._work = None
        self._refine_work = None
        self._synth_tables = {}

    # -- reference set ---------------------------------------------------------------------------
    def set_refs(self, refs, window, penalty):
        if self.torch.is_tensor(refs):   # (a device tensor, e.g. `MedoidResult.refs`: the set is uploaded from the host)
            refs = refs.detach().cpu().numpy()
        refs = np.ascontiguousarray(refs, dtype=np.float64)
        if refs.ndim != 2:
            raise ValueError("refs must be (nY, L)")
        self.nY, self.K = refs.shape
        if self.params.barcode_num_events != self.K:
            raise ValueError(
                f"barcode_num_events ({self.params.barcode_num_events}) must equal the reference length ({self.K})")
        _marshal.set_refs(self.ctx, refs, window, penalty)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.tdev).cuda_stream)

    # -- the rows of a call: float32 `sig`, or an AdcShard ------------------------------------------------
    def _rows(self, name, sig, offsets, stride, max_len, n):
        """(entry, the arguments between the context and a_start) of device entry ``name`` for these rows: the float32 entry
        itself, or its ``_adc_dev`` twin for an `AdcShard` (whose descriptor stays alive in the returned tuple)."""
        if not isinstance(sig, AdcShard):
            return getattr(self.L, name), (_dp(sig), _dp(offsets), None, int(stride), int(max_len), n)
        if offsets is not None or stride:
            raise ValueError("an AdcShard carries its own offsets / stride")
        if sig.n_reads != n:
            raise ValueError(f"the AdcShard holds {sig.n_reads} reads, a_start {n}")
        desc = sig.to_c()
        return getattr(self.L, name[:-len("_dev")] + "_adc_dev"), (C.byref(desc), int(max_len), n)

    def _work_for(self, sig, n, max_len, K, refine):
        """the d_work tensor of a call with these rows (grown on demand): the float32 entries size it by n, the int16 twins by
        their largest slice (wdx_demux[_refine]_adc_workspace_bytes)"""
        if isinstance(sig, AdcShard):
            f = self.L.wdx_demux_refine_adc_workspace_bytes if refine else self.L.wdx_demux_adc_workspace_bytes
            need = int(f(self.ctx.handle, n, int(max_len), K))
        else:
            need = int((self.L.wdx_demux_refine_workspace_bytes if refine else self.L.wdx_demux_workspace_bytes)(n, K))
        attr = "_refine_work" if refine else "_work"
        w = getattr(self, attr)
        if w is None or w.numel() < need:
            w = self.torch.empty(need, dtype=self.torch.uint8, device=self.tdev)
            setattr(self, attr, w)
        return w

    def adc_staging_bytes(self, n, max_len, refine=False):
        """device bytes of the float32 staging block an `AdcShard` call of n reads needs on this engine's context"""
        return int(self.L.wdx_adc_dev_staging_bytes(self.ctx.handle, int(n), int(max_len), int(bool(refine))))

    # -- fused path --------------------------------------------------------------------------------
    def demux(self, sig, a_start, a_end, *, offsets=None, stride=0, max_len: int, ok=None,
              counts=None, want_fpt=False, out: Optional[DemuxResult] = None) -> DemuxResult:
        """sig: float32 device tensor, packed (with int64 ``offsets`` of n+1) or a (n, stride)
        minibatch -- or an `AdcShard`; a_start/a_end: int32 device tensors.  Enqueues on the current stream."""
        torch = self.torch
        n = int(a_start.shape[0])
        if out is None:
            out = DemuxResult(
                dist=torch.empty((n, self.nY), dtype=torch.float32, device=self.tdev),
                call=torch.empty(n, dtype=torch.int32, device=self.tdev),
                status=torch.empty(n, dtype=torch.int32, device=self.tdev),
                counts=counts if counts is not None else torch.zeros(self.nY + 1, dtype=torch.int64, device=self.tdev),
                fpt=torch.empty((n, self.K), dtype=torch.float64, device=self.tdev) if want_fpt else None,
            )
        pc = self.params.to_c()
        entry, rows = self._rows("wdx_demux_dev", sig, offsets, stride, max_len, n)
        _lib.check(entry(
            self.ctx.handle, *rows,
            _dp(a_start), _dp(a_end), _dp(ok), C.byref(pc), _dp(out.fpt), None, None,
            _dp(out.status), _dp(out.dist), _dp(out.call), _dp(out.counts), _dp(self._work_for(sig, n, max_len, self.K, False)),
            self._stream()))
        return out

    # -- boundary detection ahead of every entry ----------------------------------------------------
    def detect(self, sig, *, offsets=None, stride=0, row_len=None, params: Optional[DetectParams] = None,
               want_info: bool = False) -> DetectResult:
        """Adapter boundaries of device-resident reads (wdx_detect_rows; an `AdcShard`: wdx_detect_rows_adc, bit-identical on
        the calibrated rows): float32 ``sig`` as a (n, stride) minibatch with a NaN tail (``stride`` defaults to its second
        dimension), with int32 ``row_len`` (n,), or packed with int64 ``offsets`` of n + 1 entries.  The result's tensors go
        straight into `demux` and its kin: ``d = eng.detect(sig); eng.demux(sig, d.a_start, d.a_end, ok=d.ok, ...)``.
        The engine's own rule; parity with ADAPTed unpinned; accuracy on real reads unmeasured.  Enqueues on the current stream."""
        torch = self.torch
        pc = (params or DetectParams()).to_c()
        if isinstance(sig, AdcShard):
            if offsets is not None or stride or row_len is not None:
                raise ValueError("an AdcShard carries its own offsets / stride / row_len")
            n = sig.n_reads
        else:
            if sig.dtype != torch.float32 or not sig.is_contiguous() or not sig.is_cuda:
                raise ValueError("sig must be a contiguous float32 device tensor (or an AdcShard)")
            if offsets is not None:
                # (the kernel reads n + 1 int64 entries at this address)
                if (offsets.dtype != torch.int64 or offsets.dim() != 1 or int(offsets.numel()) < 1 or not offsets.is_contiguous()
                        or not offsets.is_cuda):
                    raise ValueError("offsets must be a contiguous int64 device tensor of n + 1 entries")
                n = int(offsets.shape[0]) - 1
            else:
                if not stride:
                    if sig.dim() != 2:
                        raise ValueError("packed reads need `offsets`, strided ones a 2-D `sig` or `stride`")
                    stride = int(sig.shape[1])
                n = int(sig.numel()) // int(stride) if sig.dim() != 2 else int(sig.shape[0])
                if int(sig.numel()) < n * int(stride):
                    raise ValueError(f"sig holds {int(sig.numel())} samples, {n} rows of {stride} need more")
            if row_len is not None and (row_len.dtype != torch.int32 or tuple(row_len.shape) != (n,) or not row_len.is_cuda):
                raise ValueError("row_len must be an int32 device tensor with one entry per read")
        out = DetectResult(
            a_start=torch.empty(n, dtype=torch.int32, device=self.tdev), a_end=torch.empty(n, dtype=torch.int32, device=self.tdev),
            ok=torch.empty(n, dtype=torch.uint8, device=self.tdev), code=torch.empty(n, dtype=torch.int32, device=self.tdev),
            info=torch.empty((n, 4), dtype=torch.int32, device=self.tdev) if want_info else None,
            gain=torch.empty(n, dtype=torch.float64, device=self.tdev) if want_info else None)
        outs = (_dp(out.a_start), _dp(out.a_end), _dp(out.ok), _dp(out.code), _dp(out.info), _dp(out.gain), self._stream())
        if isinstance(sig, AdcShard):
            desc = sig.to_c()
            _lib.check(self.L.wdx_detect_rows_adc(self.ctx.handle, C.byref(desc), n, C.byref(pc), *outs))
        else:
            _lib.check(self.L.wdx_detect_rows(self.ctx.handle, _dp(sig), _dp(offsets), _dp(row_len), int(stride), n, C.byref(pc), *outs))
        return out

    def fingerprint(self, sig, a_start, a_end, *, offsets=None, stride=0, max_len: int, ok=None, want_stats: bool = True):
        """Fingerprint stage only -> (fpt f64 (n,K), dwell i64 (n,K), stats f64 (n,6) or None, status i32)."""
        torch = self.torch
        n = int(a_start.shape[0])
        fpt = torch.empty((n, self.K), dtype=torch.float64, device=self.tdev)
        dwell = torch.empty((n, self.K), dtype=torch.int64, device=self.tdev)
        stats = torch.empty((n, 6), dtype=torch.float64, device=self.tdev) if want_stats else None
        status = torch.empty(n, dtype=torch.int32, device=self.tdev)
        pc = self.params.to_c()
        entry, rows = self._rows("wdx_fingerprint_dev", sig, offsets, stride, max_len, n)
        _lib.check(entry(
            self.ctx.handle, *rows, _dp(a_start),
            _dp(a_end), _dp(ok), C.byref(pc), _dp(fpt), _dp(dwell), _dp(stats), _dp(status),
            self._stream()))
        return fpt, dwell, stats, status

    def fingerprint_refine(self, sig, a_start, a_end, refine, *, offsets=None, stride=0, max_len: int, ok=None):
        """Consensus-refinement branch on device-resident reads (wdx_fingerprint_refine_dev) ->
        (fpt f64 (n,K), dwell i64 (n,K), stats f64 (n,6), refine_idx i32 (n,3), status i32), K = refine.barcode_keep_events."""
        torch = self.torch
        n = int(a_start.shape[0])
        if not isinstance(sig, AdcShard) and offsets is None and not stride:
            if sig.dim() != 2:
                raise ValueError("packed reads need `offsets`, a minibatch needs 2-D `sig` or `stride`")
            stride = int(sig.shape[1])     # (stride 0 would make every row alias row 0)
        K = int(refine.barcode_keep_events)
        fpt = torch.empty((n, K), dtype=torch.float64, device=self.tdev)
        dwell = torch.empty((n, K), dtype=torch.int64, device=self.tdev)
        stats = torch.empty((n, 6), dtype=torch.float64, device=self.tdev)
        idx = torch.empty((n, 3), dtype=torch.int32, device=self.tdev)
        status = torch.empty(n, dtype=torch.int32, device=self.tdev)
        pc = self.params.to_c()
        rc = refine.to_c()
        entry, rows = self._rows("wdx_fingerprint_refine_dev", sig, offsets, stride, max_len, n)
        with self.ctx.refine_options_for_call(refine):   # (refine.optimal_cpts -> WDX_OPT_REFINE_OPTIMAL_CPTS for this call)
            _lib.check(entry(
                self.ctx.handle, *rows, _dp(a_start), _dp(a_end), _dp(ok),
                C.byref(pc), C.byref(rc), _dp(fpt), _dp(dwell), _dp(stats), _dp(idx), _dp(status), self._stream()))
        return fpt, dwell, stats, idx, status

    def demux_refine(self, sig, a_start, a_end, refine, *, offsets=None, stride=0, max_len: int, ok=None, counts=None):
        """`demux` with the consensus-refinement branch in front (wdx_demux_refine_dev): refine fingerprint -> DTW -> call
        -> histogram on the current stream; ``refine.barcode_keep_events`` must equal the reference length.  Returns
        (DemuxResult with fpt, dwell i64 (n,K), stats f64 (n,6), refine_idx i32 (n,3))."""
        torch = self.torch
        n = int(a_start.shape[0])
        if not isinstance(sig, AdcShard) and offsets is None and not stride:
            if sig.dim() != 2:
                raise ValueError("packed reads need `offsets`, a minibatch needs 2-D `sig` or `stride`")
            stride = int(sig.shape[1])
        K = int(refine.barcode_keep_events)
        out = DemuxResult(
            dist=torch.empty((n, self.nY), dtype=torch.float32, device=self.tdev),
            call=torch.empty(n, dtype=torch.int32, device=self.tdev),
            status=torch.empty(n, dtype=torch.int32, device=self.tdev),
            counts=counts if counts is not None else torch.zeros(self.nY + 1, dtype=torch.int64, device=self.tdev),
            fpt=torch.empty((n, K), dtype=torch.float64, device=self.tdev))
        dwell = torch.empty((n, K), dtype=torch.int64, device=self.tdev)
        stats = torch.empty((n, 6), dtype=torch.float64, device=self.tdev)
        idx = torch.empty((n, 3), dtype=torch.int32, device=self.tdev)
        work = self._work_for(sig, n, max_len, K, True)
        pc, rc = self.params.to_c(), refine.to_c()
        entry, rows = self._rows("wdx_demux_refine_dev", sig, offsets, stride, max_len, n)
        with self.ctx.refine_options_for_call(refine):
            _lib.check(entry(
                self.ctx.handle, *rows, _dp(a_start), _dp(a_end), _dp(ok),
                C.byref(pc), C.byref(rc), _dp(out.fpt), _dp(dwell), _dp(stats), _dp(idx), _dp(out.status), _dp(out.dist),
                _dp(out.call), _dp(out.counts), _dp(work), self._stream()))
        return out, dwell, stats, idx

    def dtw(self, X, want_argmin=True, out=None):
        """Device DTW of (n, L) float64 rows against the resident refs.  ``out=(dist, argmin)`` reuses the
        caller's device tensors (float32 (n, nY), int32 (n,) or None) instead of allocating."""
        torch = self.torch
        n = int(X.shape[0])
        if out is not None:
            dist, am = out
            if tuple(dist.shape) != (n, self.nY) or dist.dtype != torch.float32 or not dist.is_contiguous():
                raise ValueError("out[0] must be a contiguous float32 (n, nY) device tensor")
            if am is not None and (tuple(am.shape) != (n,) or am.dtype != torch.int32):
                raise ValueError("out[1] must be an int32 (n,) device tensor")
        else:
            dist = torch.empty((n, self.nY), dtype=torch.float32, device=self.tdev)
            am = torch.empty(n, dtype=torch.int32, device=self.tdev) if want_argmin else None
        _lib.check(self.L.wdx_dtw_matrix_dev(self.ctx.handle, _dp(X), n, _dp(dist), _dp(am), self._stream()))
        return dist, am

    # -- nearest-reference calls with reference labels, margin and rejection (wdx_nearest_dev; include/wdx.h states the rule) ---
    def _rule_args(self, labels, n_labels, min_margin, max_dist):
        """(labels int32 device tensor or None, G, min_margin / max_dist float32 device tensors or None).  Host arrays are
        checked in full and uploaded; device tensors are checked for dtype and length (labels in 0 .. G-1 is then the
        caller's precondition, and ``n_labels`` must be given)."""
        torch = self.torch
        if torch.is_tensor(labels):
            if labels.dtype != torch.int32 or tuple(labels.shape) != (self.nY,) or not labels.is_contiguous():
                raise ValueError(f"labels must be a contiguous int32 ({self.nY},) tensor")
            if n_labels is None:
                raise ValueError("device labels need n_labels")
            G = _nearest.n_labels_of(self.nY, None, n_labels)
            if G < 1:
                raise ValueError(f"n_labels must be at least 1, not {G}")
            lab = labels.to(self.tdev)
        else:
            lab, G = _nearest.host_labels(self.nY, labels, n_labels)
            lab = None if lab is None else torch.from_numpy(lab).to(self.tdev)
        thr = []
        for name, t in (("min_margin", min_margin), ("max_dist", max_dist)):
            if torch.is_tensor(t):
                if t.dtype != torch.float32 or tuple(t.shape) != (G,) or not t.is_contiguous():
                    raise ValueError(f"{name} must be a contiguous float32 ({G},) tensor")
                thr.append(t.to(self.tdev))
            else:
                t = _nearest.host_threshold(name, t, G)
                thr.append(None if t is None else torch.from_numpy(t).to(self.tdev))
        return lab, G, thr[0], thr[1]

    def _rule_counts(self, counts, G):
        torch = self.torch
        if counts is None:
            return torch.zeros(G + 1, dtype=torch.int64, device=self.tdev)
        if counts.dtype != torch.int64 or tuple(counts.shape) != (G + 1,) or not counts.is_contiguous():
            raise ValueError(f"counts must be a contiguous int64 ({G + 1},) device tensor")
        return counts

    def nearest(self, X, labels=None, n_labels=None, min_margin=None, max_dist=None, want_dist=False, counts=None, status=None):
        """The nearest-reference rule on device fingerprints X (n, L) float64 against the resident refs (wdx_nearest_dev):
        ``labels`` one label per reference (None: the identity), ``min_margin`` / ``max_dist`` a scalar or one threshold per
        label, ``status`` an optional int32 (n,) device tensor (a read whose status is not 0 is called -1).  Returns a
        `NearestResult`; without ``want_dist`` no (n, nY) matrix is allocated.  Enqueues on the current stream."""
        torch = self.torch
        if X.dtype != torch.float64 or X.dim() != 2 or int(X.shape[1]) != self.K or not X.is_contiguous():
            raise ValueError(f"X must be a contiguous float64 (n, {self.K}) device tensor")
        n = int(X.shape[0])
        lab, G, mm, md = self._rule_args(labels, n_labels, min_margin, max_dist)
        out = NearestResult(call=torch.empty(n, dtype=torch.int32, device=self.tdev),
                            best=torch.empty((n, 2), dtype=torch.float32, device=self.tdev), status=status,
                            counts=self._rule_counts(counts, G),
                            dist=torch.empty((n, self.nY), dtype=torch.float32, device=self.tdev) if want_dist else None)
        _lib.check(self.L.wdx_nearest_dev(self.ctx.handle, _dp(X), n, _dp(status), _dp(lab), G, _dp(mm), _dp(md), _dp(out.dist),
                                          _dp(out.call), _dp(out.best), _dp(out.counts), self._stream()))
        return out

    # -- reference signals from labelled fingerprints (wdx_medoids_device; include/wdx.h states the rule) ---------------------
    def medoids(self, X, labels, n_labels=None, *, window, penalty, status=None, want_cost=False):
        """The medoid of every label among the device fingerprints X (n, L) float64 -- e.g. what `fingerprint` returned for
        labelled training reads: ``labels`` one HOST integer per row in 0 .. G-1 (-1: the row takes no part), ``status`` an
        optional int32 (n,) device tensor (a row whose status is not 0 is no member, like a row with a sample that is not
        finite).  Returns a `MedoidResult` of device tensors; ``set_refs(res.refs, window, penalty)`` makes the medoids the
        resident reference set (this call itself leaves it alone).  Enqueues on the current stream."""
        torch = self.torch
        if not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 or int(X.shape[1]) < 1 or not X.is_contiguous():
            raise ValueError("X must be a contiguous float64 (n, L) device tensor with L >= 1")
        n, L = int(X.shape[0]), int(X.shape[1])
        lab, G = _medoids.host_labels(n, labels, n_labels)
        if status is not None and (not torch.is_tensor(status) or status.dtype != torch.int32 or tuple(status.shape) != (n,)
                                   or not status.is_contiguous()):
            raise ValueError(f"status must be a contiguous int32 ({n},) device tensor")
        out = MedoidResult(index=torch.empty(G, dtype=torch.int64, device=self.tdev),
                           refs=torch.empty((G, L), dtype=torch.float64, device=self.tdev),
                           count=torch.empty(G, dtype=torch.int64, device=self.tdev),
                           medoid_cost=torch.empty(G, dtype=torch.float64, device=self.tdev),
                           cost=torch.empty(n, dtype=torch.float64, device=self.tdev) if want_cost else None)
        _lib.check(self.L.wdx_medoids_device(self.ctx.handle, _dp(X), n, L, _lib.ptr(lab), G, _dp(status),
                                             int(window) if window else 0, float(penalty) if penalty else 0.0, _dp(out.index),
                                             _dp(out.medoid_cost), _dp(out.count), _dp(out.cost), _dp(out.refs), self._stream()))
        return out

    # -- barycenter reference signals (wdx_dba_step_device; include/wdx.h states the rule) -------------------------------------
    def dba_step(self, X, labels, centres, n_labels=None, *, window, penalty, status=None, want_cost=False, want_runs=False):
        """One step of DTW barycenter averaging on the device fingerprints X (n, L) float64: ``labels`` one HOST integer per row
        (-1: the row takes no part), ``centres`` a float64 (G, L) device tensor, ``status`` an optional int32 (n,) device tensor.
        Returns a `DbaResult` of device tensors: every centre point becomes the mean of the samples its label's members match
        to it; ``inertia`` is the summed cost of the centres given.  The engine's own rule, bit for bit; parity with
        dtaidistance's DBA unpinned.  Nothing resident is read or changed.  Enqueues on the current stream."""
        torch = self.torch
        if not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 or int(X.shape[1]) < 1 or not X.is_contiguous():
            raise ValueError("X must be a contiguous float64 (n, L) device tensor with L >= 1")
        n, L = int(X.shape[0]), _medoids.dba_length(X.shape[1])
        if n_labels is None and torch.is_tensor(centres) and centres.dim() == 2:
            n_labels = int(centres.shape[0])
        lab, G = _medoids.host_labels(n, labels, n_labels, max_group=False)
        if (not torch.is_tensor(centres) or centres.dtype != torch.float64 or tuple(centres.shape) != (G, L)
                or not centres.is_contiguous()):
            raise ValueError(f"centres must be a contiguous float64 ({G}, {L}) device tensor")
        if status is not None and (not torch.is_tensor(status) or status.dtype != torch.int32 or tuple(status.shape) != (n,)
                                   or not status.is_contiguous()):
            raise ValueError(f"status must be a contiguous int32 ({n},) device tensor")
        out = DbaResult(centres=torch.empty((G, L), dtype=torch.float64, device=self.tdev),
                        count=torch.empty(G, dtype=torch.int64, device=self.tdev),
                        inertia=torch.empty(G, dtype=torch.float64, device=self.tdev),
                        cost=torch.empty(n, dtype=torch.float64, device=self.tdev) if want_cost else None,
                        runs=torch.empty((n, L, 2), dtype=torch.int32, device=self.tdev) if want_runs else None)
        _lib.check(self.L.wdx_dba_step_device(self.ctx.handle, _dp(X), n, L, _lib.ptr(lab), G, _dp(status), _dp(centres),
                                              int(window) if window else 0, float(penalty) if penalty else 0.0, _dp(out.centres),
                                              _dp(out.count), _dp(out.inertia), _dp(out.cost), _dp(out.runs), self._stream()))
        return out

    def barycenters(self, X, labels, n_labels=None, *, window, penalty, status=None, init=None, n_iter=10):
        """(centres (G, L) float64, count (G,) int64, inertia (steps, G) float64, device tensors): at most ``n_iter`` steps of
        `dba_step` from ``init`` (None: `medoids(...).refs`), stopping early when a step returns every centre bit-identical to
        its input (one host read of a flag per step).  Row k of ``inertia`` belongs to the centres step k received.
        ``set_refs(centres, window, penalty)`` makes them the resident reference set."""
        torch = self.torch
        steps = _medoids.n_iterations(n_iter)
        if init is None:
            init = self.medoids(X, labels, n_labels, window=window, penalty=penalty, status=status).refs
        C0, hist, count = init, [], None
        for _ in range(steps):
            res = self.dba_step(X, labels, C0, n_labels, window=window, penalty=penalty, status=status)
            hist.append(res.inertia)
            count = res.count
            same = bool(torch.equal(res.centres.view(torch.int64), C0.view(torch.int64)))
            C0 = res.centres
            if same:
                break
        return C0, count, torch.stack(hist)

    # -- the training matrix of a DTW kernel machine (wdx_self_matrix_device; include/wdx.h states the rule) -------------------
    def self_distances(self, X, window=None, penalty=None, status=None, out=None):
        """float32 (n, n) device tensor: the DTW distances of the device fingerprints X (n, L) float64 against themselves, each
        unordered pair computed once.  ``status``: an optional int32 (n,) device tensor; a row whose status is not 0, like a
        row with a sample that is not finite, is no member, and its row and column are NaN.  ``out``: a float32 device tensor
        of n rows and at least n columns whose columns are contiguous -- a wider tensor (or a view of one) keeps its columns
        from n on, its row stride is the matrix's leading dimension.  ``window`` / ``penalty`` as for `distance_matrix_to`
        (``None``: unbanded / no penalty); the resident reference set is neither read nor changed.  Enqueues on the current
        stream."""
        torch = self.torch
        if not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 or int(X.shape[1]) < 1 or not X.is_contiguous():
            raise ValueError("X must be a contiguous float64 (n, L) device tensor with L >= 1")
        n, L = int(X.shape[0]), int(X.shape[1])
        if n > _lib.SELF_MATRIX_MAX_ROWS:
            raise NotImplementedError(f"self matrix: n = {n} rows, more than WDX_SELF_MATRIX_MAX_ROWS = {_lib.SELF_MATRIX_MAX_ROWS}: "
                                      "subsample them")
        if status is not None and (not torch.is_tensor(status) or status.dtype != torch.int32 or tuple(status.shape) != (n,)
                                   or not status.is_contiguous()):
            raise ValueError(f"status must be a contiguous int32 ({n},) device tensor")
        if out is None:
            out = torch.empty((n, n), dtype=torch.float32, device=self.tdev)
        elif (not torch.is_tensor(out) or out.dtype != torch.float32 or out.dim() != 2 or int(out.shape[0]) != n or int(out.shape[1]) < n
              or (n > 0 and int(out.shape[1]) > 1 and out.stride(1) != 1) or (n > 1 and out.stride(0) < int(out.shape[1]))):
            raise ValueError(f"out must be a float32 device tensor of {n} rows and at least {n} contiguous columns")
        ld = int(out.stride(0)) if n > 1 else max(n, int(out.shape[1]))
        _lib.check(self.L.wdx_self_matrix_device(self.ctx.handle, _dp(X), n, L, _dp(status), int(window) if window else 0,
                                                 float(penalty) if penalty else 0.0, _dp(out), ld, self._stream()))
        return out[:, :n]

    # -- fitting a kernel machine on a resident kernel matrix (wdx_svm_solve_device; include/wdx.h states the rule) ------------
    def svm_solve(self, K, problems, rows, eval_rows=None, eps=1e-3, max_iter=10_000_000):
        """`SvmSolveResult` of device tensors: a batch of binary C-SVC duals on the float32 device kernel matrix ``K`` (m rows,
        at least m contiguous columns; a view of a wider tensor keeps its row stride as the leading dimension), one workgroup
        per problem -- for callers who sweep C or the class weights over one resident ``K``.  ``problems``: a NumPy array of
        `_svm_fit.PROBLEM_DTYPE` (wdx_svm_problem); ``rows`` / ``eval_rows``: the int32 HOST lists it points into (K-row
        indices: they are checked on the host before anything is launched).  A problem of more than
        ``_lib.SVM_FIT_MAX_ROWS`` rows is NotImplementedError.  Enqueues on the current stream; does not synchronise."""
        from . import _svm_fit

        torch = self.torch
        if (not torch.is_tensor(K) or K.dtype != torch.float32 or K.dim() != 2 or int(K.shape[0]) < 1 or int(K.shape[1]) < int(K.shape[0])
                or (int(K.shape[1]) > 1 and K.stride(1) != 1) or (int(K.shape[0]) > 1 and K.stride(0) < int(K.shape[1]))):
            raise ValueError("K must be a float32 device tensor of m >= 1 rows and at least m contiguous columns")
        m = int(K.shape[0])
        ld = int(K.stride(0)) if m > 1 else int(K.shape[1])
        problems = np.ascontiguousarray(problems, dtype=_svm_fit.PROBLEM_DTYPE)
        if problems.ndim != 1:
            raise ValueError("problems must be a one-dimensional array of _svm_fit.PROBLEM_DTYPE")
        rows = np.ascontiguousarray(rows, dtype=np.int32).ravel()
        eval_rows = np.zeros(0, np.int32) if eval_rows is None else np.ascontiguousarray(eval_rows, dtype=np.int32).ravel()
        if len(problems) and (problems["n_pos"].astype(np.int64) + problems["n_neg"]).max() > _lib.SVM_FIT_MAX_ROWS:
            raise NotImplementedError(f"svm solve: a problem of {int((problems['n_pos'].astype(np.int64) + problems['n_neg']).max())} rows, "
                                      f"more than WDX_SVM_FIT_MAX_ROWS = {_lib.SVM_FIT_MAX_ROWS}")
        Q = len(problems)
        out = SvmSolveResult(alpha=torch.zeros(len(rows), dtype=torch.float64, device=self.tdev),
                             rho=torch.empty(Q, dtype=torch.float64, device=self.tdev),
                             n_iter=torch.empty(Q, dtype=torch.int64, device=self.tdev),
                             state=torch.empty(Q, dtype=torch.int32, device=self.tdev),
                             dec=torch.zeros(len(eval_rows), dtype=torch.float64, device=self.tdev))
        _lib.check(self.L.wdx_svm_solve_device(self.ctx.handle, _dp(K), m, ld, _lib.ptr(problems), Q, _lib.ptr(rows), len(rows),
                                               _lib.ptr(eval_rows), len(eval_rows), float(eps), int(max_iter), _dp(out.alpha), _dp(out.rho),
                                               _dp(out.n_iter), _dp(out.state), _dp(out.dec), self._stream()))
        return out

    # -- the kernel matrix of a kernel machine from the resident self-distance matrix (wdx_svm_kernel_device; include/wdx.h states the rule)
    def svm_kernel(self, D, gamma, pwr_dist=1, out=None):
        """float32 (m, m) device tensor ``K = exp_rule(-(gamma * D ** pwr_dist))`` of the float32 device distances ``D`` (m rows, at
        least m contiguous columns; a view of a wider tensor keeps its row stride as the leading dimension; `self_distances`
        leaves such a matrix on the device).  ``out``: a float32 device tensor of the same kind; ``out=D`` works in place.  The
        exponential is the engine's stated ``exp_rule`` (include/wdx.h) of a float64 product, not ``numpy.exp`` of a float32
        one: an entry may differ from the host route's by a few float32 ulps.  A distance of +inf gives 0, a NaN gives NaN.  Enqueues on the current stream; does not
        synchronise."""
        torch = self.torch

        def matrix(t, name):
            if (not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or int(t.shape[0]) < 1 or int(t.shape[1]) < int(t.shape[0])
                    or (int(t.shape[1]) > 1 and t.stride(1) != 1) or (int(t.shape[0]) > 1 and t.stride(0) < int(t.shape[1]))):
                raise ValueError(f"{name} must be a float32 device tensor of m >= 1 rows and at least m contiguous columns")
            return int(t.stride(0)) if int(t.shape[0]) > 1 else int(t.shape[1])

        ld = matrix(D, "D")
        m = int(D.shape[0])
        if out is None:
            out = torch.empty((m, m), dtype=torch.float32, device=self.tdev)
        ldk = matrix(out, "out")
        if int(out.shape[0]) != m:
            raise ValueError(f"out must have {m} rows, not {int(out.shape[0])}")
        if int(pwr_dist) != pwr_dist:
            raise ValueError(f"pwr_dist must be an integer, not {pwr_dist!r}")
        _lib.check(self.L.wdx_svm_kernel_device(self.ctx.handle, _dp(D), m, ld, float(gamma), int(pwr_dist), _dp(out), ldk, self._stream()))
        return out[:, :m]

    # -- cross-validated probabilities on a resident kernel matrix (_svm_cv states the plan; wdx_svm_cv_couple_device the tail) ------
    def svm_cross_val(self, K, y_idx, k, C=1.0, class_weight=None, tol=1e-3, max_iter=-1, random_state=0, cv=5, with_full=False,
                      classes=None):
        """`SvmCvResult`: ``cv``-fold out-of-fold probabilities of a precomputed-kernel SVC on the float32 device kernel matrix
        ``K`` (as for `svm_solve`) and the HOST class numbers ``y_idx`` (0 .. k-1, one per row of ``K``).  Every fold's
        one-vs-one problems, their Platt folds and, with ``with_full``, the full data's own fit are ONE `svm_solve` launch
        (`_svm_cv` states the folds and the plan); the host then fits ``probA`` / ``probB`` per fold (`_svm_fit.sigmoid_train`)
        and wdx_svm_cv_couple_device turns the held-out decision values into probabilities with the resident tail's own code.
        ``classes``: the k labels a ``class_weight`` dict names (default 0 .. k-1).  A class with fewer than ``cv`` members is
        ValueError before any device work.  The call blocks: it synchronises the current stream once, behind the solve."""
        from . import _svm_cv, _svm_fit

        torch = self.torch
        y_idx = np.asarray(y_idx)
        k = int(k)
        if y_idx.ndim != 1 or y_idx.dtype.kind not in "iu" or (len(y_idx) and (y_idx.min() < 0 or y_idx.max() >= k)):
            raise ValueError(f"y_idx must hold one class number 0 .. {k - 1} per row")
        if not 2 <= k <= _lib.SVM_MAX_CLASSES:
            raise ValueError(f"k = {k} classes (2..{_lib.SVM_MAX_CLASSES})")
        if not torch.is_tensor(K) or K.dim() != 2 or int(K.shape[0]) != len(y_idx):
            raise ValueError(f"K must be a device matrix of {len(y_idx)} rows, one per entry of y_idx")
        for name, v in (("tol", tol), ("C", C)):
            if not (np.isscalar(v) and np.isreal(v) and np.isfinite(v) and v > 0):
                raise ValueError(f"{name} must be positive and finite, not {v!r}")
        if not isinstance(random_state, (int, np.integer)) or random_state < 0:
            raise ValueError(f"random_state must be a non-negative integer, not {random_state!r}")
        classes = np.arange(k) if classes is None else np.asarray(classes)
        _svm_fit.effective_max_iter(max_iter, 0)
        p = _svm_cv.plan(y_idx, k, float(C), class_weight, classes, int(random_state), cv, with_full)
        _svm_fit.check_batch(p.batch)
        dev = self.svm_solve(K, p.batch.problems, p.batch.rows, p.batch.eval_rows, eps=float(tol),
                             max_iter=_svm_fit.effective_max_iter(max_iter, _svm_cv.largest_problem(p)))
        sol = _svm_fit.Solution(*(t.cpu().numpy() for t in (dev.alpha, dev.rho, dev.n_iter, dev.state, dev.dec)))
        parts = [_svm_cv.part_arrays(p, g, y_idx, sol) for g in range(len(p.sub))]
        off, A, B, held, held_off = _svm_cv.couple_tables(p, [a[4] for a in parts[:p.cv]], [a[5] for a in parts[:p.cv]])
        m = len(y_idx)
        prob = torch.full((m, k), float("nan"), dtype=torch.float64, device=self.tdev)
        pred = torch.full((m,), -1, dtype=torch.int32, device=self.tdev)
        conf = torch.full((m,), float("nan"), dtype=torch.float64, device=self.tdev)
        _lib.check(self.L.wdx_svm_cv_couple_device(self.ctx.handle, _dp(dev.dec), int(dev.dec.numel()), k, p.cv, _lib.ptr(off), _lib.ptr(A),
                                                _lib.ptr(B), _lib.ptr(held), _lib.ptr(held_off), m, _dp(prob), _dp(pred), _dp(conf),
                                                self._stream()))
        return SvmCvResult(prob=prob, pred_idx=pred, conf=conf, fold_of_row=p.fold_of_row, folds=parts[:p.cv], train=p.train, held=p.held,
                           fit_info=_svm_cv.fit_info(p, sol), full=parts[p.cv] if with_full else None, plan=p, solution=sol)

    # -- per-class confidence thresholds from labelled probabilities (wdx_accuracy_thresholds_device; include/wdx.h states the rule) --
    def accuracy_thresholds(self, prob, y_idx, targets=(0.99,), resolution=100):
        """``(thr (T, k) float64, kept (k, R + 1) int64, hit (k, R + 1) int64, skipped int64 ())`` device tensors: per target
        accuracy and predicted class the smallest margin ``j / R`` (j >= 1) at which the rows called that class with at least
        that margin reach the target, ``+inf`` where none does -- a row of ``thr`` is a ``thresholds=`` vector of a model.
        ``prob``: a contiguous float64 (n, k) device tensor -- what `demux_svm` / `demux_mlp` / `demux_boost` or `svm_predict`
        left on the device, or held-out probabilities; ``y_idx``: the int32 (n,) device class indices (negative: the row is
        skipped, like a row with a probability that is not finite).  ``targets``: fractions that are whole numbers of per
        mille (ValueError otherwise).  ``kept`` / ``hit``: the suffix sums the rule selects from.  Enqueues on the current
        stream; does not synchronise."""
        from . import _thresholds

        torch = self.torch
        if not torch.is_tensor(prob) or prob.dtype != torch.float64 or prob.dim() != 2 or not prob.is_contiguous():
            raise ValueError("prob must be a contiguous float64 (n, k) device tensor")
        n, k = int(prob.shape[0]), int(prob.shape[1])
        if not torch.is_tensor(y_idx) or y_idx.dtype != torch.int32 or tuple(y_idx.shape) != (n,) or not y_idx.is_contiguous():
            raise ValueError(f"y_idx must be a contiguous int32 ({n},) device tensor")
        R = int(resolution)
        _thresholds.check_sizes(k, R)
        pm = _thresholds.targets_per_mille(targets)
        thr = torch.empty((len(pm), k), dtype=torch.float64, device=self.tdev)
        kept = torch.empty((k, R + 1), dtype=torch.int64, device=self.tdev)
        hit = torch.empty((k, R + 1), dtype=torch.int64, device=self.tdev)
        skipped = torch.empty((), dtype=torch.int64, device=self.tdev)
        _lib.check(self.L.wdx_accuracy_thresholds_device(self.ctx.handle, _dp(prob), n, k, _dp(y_idx), R, _lib.ptr(pm), len(pm), _dp(thr),
                                                      _dp(kept), _dp(hit), _dp(skipped), self._stream()))
        return thr, kept, hit, skipped

    # -- training the MLP tail on a resident distance matrix (wdx_mlp_fit_device; include/wdx.h states the rule) ---------------
    def mlp_fit(self, dist, y_idx, coefs, intercepts, *, activation="relu", n_classes=None, mean=None, scale=None, order=None,
                batch_size=200, max_epochs=200, n_iter_no_change=10, learning_rate_init=1e-3, alpha=1e-4, beta_1=0.9, beta_2=0.999,
                epsilon=1e-8, tol=1e-4):
        """`_mlp_fit.FitResult` (host arrays): scikit-learn's ``MLPClassifier(solver="adam")`` trained in float32 on the float32
        device matrix ``dist`` (m rows, F contiguous columns; a view of a wider tensor keeps its row stride as the leading
        dimension) and the int32 (m,) device class indices ``y_idx``.  ``coefs`` / ``intercepts``: the HOST initial weights per
        layer (F -> hidden... -> n_classes, or one unit for two classes; `_mlp_fit.schedule` draws scikit-learn's); ``mean`` /
        ``scale``: optional HOST float64 (F,) scaler; ``order``: the optional HOST (max_epochs, m) int32 table of the epochs' row
        orders (None: unshuffled).  ``n_classes`` defaults to the output layer's width (2 for one unit).  The call blocks: it
        synchronises the current stream once per epoch.  A limit exceeded is NotImplementedError, a malformed argument
        ValueError, both before anything is launched."""
        from . import _mlp_fit

        torch = self.torch
        if (not torch.is_tensor(dist) or dist.dtype != torch.float32 or dist.dim() != 2 or int(dist.shape[0]) < 1 or int(dist.shape[1]) < 1
                or (int(dist.shape[1]) > 1 and dist.stride(1) != 1) or (int(dist.shape[0]) > 1 and dist.stride(0) < int(dist.shape[1]))):
            raise ValueError("dist must be a float32 device tensor of m >= 1 rows and F >= 1 contiguous columns")
        m, F = int(dist.shape[0]), int(dist.shape[1])
        ld = int(dist.stride(0)) if m > 1 else F
        if not torch.is_tensor(y_idx) or y_idx.dtype != torch.int32 or tuple(y_idx.shape) != (m,) or not y_idx.is_contiguous():
            raise ValueError(f"y_idx must be a contiguous int32 ({m},) device tensor")
        sizes = [F] + [int(np.shape(b)[0]) for b in intercepts]
        if len(sizes) < 2:
            raise ValueError("coefs and intercepts must hold at least one layer")
        k = int(n_classes) if n_classes is not None else (2 if sizes[-1] == 1 else sizes[-1])
        p = _mlp_fit.params_c(sizes, activation, k, batch_size, max_epochs, n_iter_no_change, learning_rate_init, alpha, beta_1, beta_2,
                              epsilon, tol)
        W, B, mean, scale, order = _mlp_fit.check_arrays(sizes, m, coefs, intercepts, mean, scale, order, int(max_epochs))
        return _mlp_fit.call(self.L.wdx_mlp_fit_device, self.ctx.handle, _dp(dist), m, ld, _dp(y_idx), p, W, B, mean, scale, order,
                             stream=self._stream())

    # -- training the boost tail on resident fingerprints (wdx_boost_fit_device; include/wdx.h states the rule) -------------------
    def boost_fit(self, X, y_idx, borders, scores, *, n_trees, depth=6, learning_rate=0.1, l2_leaf_reg=3.0, border_count=None):
        """`_boost_fit.FitTrees` (host arrays) of ``n_trees`` more oblivious trees on the float64 device fingerprints ``X`` (n rows,
        F contiguous columns; a view of a wider tensor keeps its row stride as the leading dimension), the int32 (n,) device class
        indices ``y_idx`` and the float64 (n, k) contiguous device ``scores``, which are IN/OUT: zeros for a fresh fit, and a
        further call continues the fit -- that is how a caller looks at a validation set between blocks of trees.  ``borders``:
        the HOST list of the features' ascending float32 borders (`_boost_fit.borders` makes them from the data);
        ``border_count`` defaults to the longest of them.  `_boost_fit.trees_of` turns the result into `models.Fpt_Boost`'s
        trees.  The call blocks: it synchronises the current stream before the first tree and after the last, never in between.
        A limit exceeded is NotImplementedError, a malformed argument ValueError, both before any tree is built."""
        from . import _boost_fit

        torch = self.torch
        if (not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 or int(X.shape[0]) < 1 or int(X.shape[1]) < 1
                or (int(X.shape[1]) > 1 and X.stride(1) != 1) or (int(X.shape[0]) > 1 and X.stride(0) < int(X.shape[1]))):
            raise ValueError("X must be a float64 device tensor of n >= 1 rows and F >= 1 contiguous columns")
        n, F = int(X.shape[0]), int(X.shape[1])
        ld = int(X.stride(0)) if n > 1 else F
        if not torch.is_tensor(y_idx) or y_idx.dtype != torch.int32 or tuple(y_idx.shape) != (n,) or not y_idx.is_contiguous():
            raise ValueError(f"y_idx must be a contiguous int32 ({n},) device tensor")
        if (not torch.is_tensor(scores) or scores.dtype != torch.float64 or scores.dim() != 2 or int(scores.shape[0]) != n
                or not scores.is_contiguous()):
            raise ValueError(f"scores must be a contiguous float64 ({n}, k) device tensor")
        if len(borders) != F:
            raise ValueError(f"borders must hold one array per feature: {F}, not {len(borders)}")
        flat, nb = _boost_fit.pack_borders(borders)
        if border_count is None:
            border_count = max(1, int(nb.max()))
        p = _boost_fit.params_c(F, int(scores.shape[1]), n_trees, depth, border_count, learning_rate, l2_leaf_reg)
        return _boost_fit.call(self.L.wdx_boost_fit_device, self.ctx.handle, _dp(X), n, ld, _dp(y_idx), flat, nb, p, _dp(scores),
                               stream=self._stream())

    # -- is a labelled set any good (wdx_self_nearest_device; include/wdx.h states the rule) -----------------------------------
    def loo_nearest(self, X, labels=None, *, window, penalty, status=None):
        """`LooResult` of device tensors: per row of the device fingerprints X (n, L) float64 the nearest other row of its own
        label and the nearest row of any other label, with the distances -- the self matrix's tile walk without the (n, n)
        matrix.  ``labels``: an optional int32 (n,) device tensor (-1: the row takes no part; None: every row has label 0);
        ``status``: an optional int32 (n,) device tensor (a row whose status is not 0, like a row with a sample that is not
        finite, is no member: nn -1, best NaN).  `parallel_distances.loo_summary` reads the result on the host.  Nothing
        resident is read or changed.  Enqueues on the current stream; does not synchronise."""
        torch = self.torch
        if not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 or int(X.shape[1]) < 1 or not X.is_contiguous():
            raise ValueError("X must be a contiguous float64 (n, L) device tensor with L >= 1")
        n, L = int(X.shape[0]), int(X.shape[1])
        if n > _lib.SELF_MATRIX_MAX_ROWS:
            raise NotImplementedError(f"self nearest: n = {n} rows, more than WDX_SELF_MATRIX_MAX_ROWS = {_lib.SELF_MATRIX_MAX_ROWS}: "
                                      "subsample them")
        for name, t in (("labels", labels), ("status", status)):
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous int32 ({n},) device tensor")
        out = LooResult(nn=torch.empty((n, 2), dtype=torch.int32, device=self.tdev),
                        best=torch.empty((n, 2), dtype=torch.float32, device=self.tdev))
        _lib.check(self.L.wdx_self_nearest_device(self.ctx.handle, _dp(X), n, L, _dp(labels), _dp(status), int(window) if window else 0,
                                                  float(penalty) if penalty else 0.0, _dp(out.nn), _dp(out.best), self._stream()))
        return out

    def demux_nearest(self, sig, a_start, a_end, *, offsets=None, stride=0, max_len: int, ok=None, labels=None, n_labels=None,
                      min_margin=None, max_dist=None, want_dist=False, want_fpt=False, counts=None):
        """`demux` with the nearest-reference rule in the argmin's place (wdx_demux_nearest_dev): raw float32 rows ->
        fingerprint -> DTW -> label of the nearest reference, margin, rejection, per-label histogram.  Returns a
        `NearestResult` (``status`` the reads' own).  An `AdcShard` is not accepted here."""
        torch = self.torch
        if isinstance(sig, AdcShard):
            raise NotImplementedError("demux_nearest takes float32 rows (no int16 twin of wdx_demux_nearest_dev exists)")
        n = int(a_start.shape[0])
        lab, G, mm, md = self._rule_args(labels, n_labels, min_margin, max_dist)
        out = NearestResult(call=torch.empty(n, dtype=torch.int32, device=self.tdev),
                            best=torch.empty((n, 2), dtype=torch.float32, device=self.tdev),
                            status=torch.empty(n, dtype=torch.int32, device=self.tdev), counts=self._rule_counts(counts, G),
                            dist=torch.empty((n, self.nY), dtype=torch.float32, device=self.tdev) if want_dist else None,
                            fpt=torch.empty((n, self.K), dtype=torch.float64, device=self.tdev) if want_fpt else None)
        pc = self.params.to_c()
        _lib.check(self.L.wdx_demux_nearest_dev(
            self.ctx.handle, _dp(sig), _dp(offsets), None, int(stride), int(max_len), n, _dp(a_start), _dp(a_end), _dp(ok),
            C.byref(pc), _dp(out.fpt), None, None, _dp(out.status), _dp(lab), G, _dp(mm), _dp(md), _dp(out.dist), _dp(out.call),
            _dp(out.best), _dp(out.counts), _dp(self._work_for(sig, n, max_len, self.K, False)), self._stream()))
        return out

    # -- classifier tails: SVM, MLP (DTW_MLP), boosted trees (Fpt_Boost; 4.8) --------
    def _set_model(self, model, kind):
        """Upload ``model`` and record it as the owner of the context's ``kind`` slot."""
        if kind != "boost" and model._X.shape != (self.nY, self.K):
            raise ValueError(f"the {kind.upper()}'s training set must be the engine's reference set")
        setattr(self, f"_{kind}_model", model)   # keeps the host arrays alive during the upload
        setattr(self.ctx, f"_{kind}_owner", None)
        _marshal.set_model(self.ctx, model)
        setattr(self.ctx, f"_{kind}_owner", model)

    def _tail_predict(self, entry, k, dist, *extra):
        """``entry`` (wdx_{svm,mlp}_predict_dev) on a device distance matrix; ``extra``: arguments between conf and the stream."""
        torch = self.torch
        n = int(dist.shape[0])
        prob = torch.empty((n, k), dtype=torch.float64, device=self.tdev)
        pred = torch.empty(n, dtype=torch.int32, device=self.tdev)
        conf = torch.empty(n, dtype=torch.float64, device=self.tdev)
        _lib.check(entry(self.ctx.handle, _dp(dist), n, _dp(prob), _dp(pred), _dp(conf), *extra, self._stream()))
        return prob, pred, conf

    def _demux_tail(self, entry, k, sig, a_start, a_end, offsets, stride, max_len, ok, want_dist, want_fpt, block_rows, out,
                    *extra):
        """``entry`` (the name of wdx_demux_{svm,mlp}_dev) on raw rows; ``extra``: arguments between conf and the workspace."""
        torch = self.torch
        n = int(a_start.shape[0])
        if out is None:
            out = (torch.empty((n, k), dtype=torch.float64, device=self.tdev),
                   torch.empty(n, dtype=torch.int32, device=self.tdev),
                   torch.empty(n, dtype=torch.float64, device=self.tdev),
                   torch.empty(n, dtype=torch.int32, device=self.tdev),
                   torch.empty((n, self.nY), dtype=torch.float32, device=self.tdev) if want_dist else None,
                   torch.empty((n, self.K), dtype=torch.float64, device=self.tdev) if want_fpt else None)
        prob, pred, conf, status, dist, fpt = out
        pc = self.params.to_c()
        entry, rows = self._rows(entry, sig, offsets, stride, max_len, n)
        _lib.check(entry(
            self.ctx.handle, *rows, _dp(a_start), _dp(a_end), _dp(ok),
            C.byref(pc), _dp(fpt), _dp(status), _dp(dist), _dp(prob), _dp(pred), _dp(conf), *extra,
            _dp(self._work_for(sig, n, max_len, self.K, False)), int(block_rows), self._stream()))
        return out

    def set_svm(self, model):
        """``model``: a warpdemux_amd.models.DTW_SVM whose ``_X`` is the resident reference set."""
        self._set_model(model, "svm")
        self.n_classes = model.n_classes

    def svm_predict(self, dist):
        """(prob f64 (n,k), pred i32 (n,), conf f64 (n,)) from a device (n, nY) float32 distance matrix:
        models/dtw_svm.py:90-93 + models/utils.py:45-61."""
        return self._tail_predict(self.L.wdx_svm_predict_dev, self.n_classes, dist)

    def demux_svm(self, sig, a_start, a_end, *, offsets=None, stride=0, max_len: int, ok=None, want_dist=False,
                  want_fpt=False, block_rows: int = 0, out=None):
        """The shipped models' whole path, device-resident (wdx_demux_svm_dev): raw rows -> fingerprint -> DTW against
        the resident training set -> SVM tail.  Returns (prob f64 (n,k), pred i32 (n,), conf f64 (n,), status i32 (n,),
        dist f32 (n,nY) or None, fpt f64 (n,K) or None); ``out`` = such a tuple from an earlier call is reused."""
        return self._demux_tail("wdx_demux_svm_dev", self.n_classes, sig, a_start, a_end, offsets, stride, max_len, ok,
                                want_dist, want_fpt, block_rows, out)

    def set_mlp(self, model):
        """``model``: a warpdemux_amd.models.DTW_MLP whose ``_X`` is the resident reference set."""
        self._set_model(model, "mlp")
        self.mlp_classes = model.k

    def mlp_predict(self, dist, n_nonfinite=None):
        """(prob f64 (n,k), pred i32 (n,), conf f64 (n,)) from a device (n, nY) float32 distance matrix (wdx_mlp_predict_dev);
        ``n_nonfinite``: optional int64 (1,) device tensor, incremented by the rows with a non-finite input."""
        return self._tail_predict(self.L.wdx_mlp_predict_dev, self.mlp_classes, dist, _dp(n_nonfinite))

    def demux_mlp(self, sig, a_start, a_end, *, offsets=None, stride=0, max_len: int, ok=None, want_dist=False,
                  want_fpt=False, block_rows: int = 0, n_nonfinite=None, out=None):
        """demux_svm with the MLP tail (wdx_demux_mlp_dev): raw rows -> fingerprint -> DTW row blocks -> MLP tail.  Returns
        (prob f64 (n,k), pred i32 (n,), conf f64 (n,), status i32 (n,), dist f32 (n,nY) or None, fpt f64 (n,K) or None)."""
        return self._demux_tail("wdx_demux_mlp_dev", self.mlp_classes, sig, a_start, a_end, offsets, stride, max_len, ok,
                                want_dist, want_fpt, block_rows, out, _dp(n_nonfinite))

    def set_boost(self, model):
        """``model``: a warpdemux_amd.models.Fpt_Boost; its features are the fingerprint's K columns.  Needs no reference set:
        the engine's own stays as it is."""
        self._set_model(model, "boost")
        self.boost_classes, self.boost_dim, self.boost_features = model.k, model.dim, model.n_features

    def boost_predict(self, fpt, status=None, want_raw=False):
        """(prob f64 (n,k), pred i32 (n,), conf f64 (n,)[, raw f64 (n,dim)]) from device (n, K) float64 fingerprints
        (wdx_boost_predict_dev); ``status``: optional int32 (n,) device tensor, rows with a non-zero status get -1 / NaN."""
        torch = self.torch
        n = int(fpt.shape[0])
        if fpt.dtype != torch.float64 or not fpt.is_contiguous() or fpt.dim() != 2 or int(fpt.shape[1]) != self.boost_features:
            raise ValueError(f"fpt must be a contiguous float64 (n, {self.boost_features}) device tensor")
        prob = torch.empty((n, self.boost_classes), dtype=torch.float64, device=self.tdev)
        pred = torch.empty(n, dtype=torch.int32, device=self.tdev)
        conf = torch.empty(n, dtype=torch.float64, device=self.tdev)
        raw = torch.empty((n, self.boost_dim), dtype=torch.float64, device=self.tdev) if want_raw else None
        _lib.check(self.L.wdx_boost_predict_dev(self.ctx.handle, _dp(fpt), _dp(status), n, _dp(raw), _dp(prob), _dp(pred),
                                                _dp(conf), self._stream()))
        return (prob, pred, conf, raw) if want_raw else (prob, pred, conf)

    def demux_boost(self, sig, a_start, a_end, refine=None, *, offsets=None, stride=0, max_len: int, ok=None, want_fpt=False,
                    want_raw=False):
        """The tRNA flow in one call (wdx_demux_boost_dev): raw rows -> fingerprint (with ``refine``, a RefineParams: the
        consensus-refinement branch, K = refine.barcode_keep_events; else K = params.barcode_num_events) -> boost tail, on
        the current stream.  Returns (prob f64 (n,k), pred i32 (n,), conf f64 (n,), status i32 (n,), refine_idx i32 (n,3) or
        None, fpt f64 (n,K) or None, raw f64 (n,dim) or None)."""
        torch = self.torch
        n = int(a_start.shape[0])
        if not isinstance(sig, AdcShard) and offsets is None and not stride:
            if sig.dim() != 2:
                raise ValueError("packed reads need `offsets`, a minibatch needs 2-D `sig` or `stride`")
            stride = int(sig.shape[1])
        K = int(refine.barcode_keep_events) if refine is not None else int(self.params.barcode_num_events)
        prob = torch.empty((n, self.boost_classes), dtype=torch.float64, device=self.tdev)
        pred = torch.empty(n, dtype=torch.int32, device=self.tdev)
        conf = torch.empty(n, dtype=torch.float64, device=self.tdev)
        status = torch.empty(n, dtype=torch.int32, device=self.tdev)
        idx = torch.empty((n, 3), dtype=torch.int32, device=self.tdev) if refine is not None else None
        fpt = torch.empty((n, K), dtype=torch.float64, device=self.tdev) if want_fpt else None
        raw = torch.empty((n, self.boost_dim), dtype=torch.float64, device=self.tdev) if want_raw else None
        # (float32 rows: the refine size, as always; a shard: the size of the branch the call takes, whose slices it is planned by)
        work = self._work_for(sig, n, max_len, K, refine is not None or not isinstance(sig, AdcShard))
        pc = self.params.to_c()
        rc = refine.to_c() if refine is not None else None
        entry, rows = self._rows("wdx_demux_boost_dev", sig, offsets, stride, max_len, n)
        with self.ctx.refine_options_for_call(refine):
            _lib.check(entry(
                self.ctx.handle, *rows, _dp(a_start), _dp(a_end), _dp(ok),
                C.byref(pc), C.byref(rc) if rc is not None else None, _dp(fpt), _dp(idx), _dp(status), _dp(raw), _dp(prob),
                _dp(pred), _dp(conf), _dp(work), self._stream()))
        return prob, pred, conf, status, idx, fpt, raw

    # -- synthetic inputs, generated in HBM ----------------------------------------------------------
    def synth_packed(self, spec: synth.SynthSpec, first_read: int, n_reads: int):
        """(sig f32[total], offsets i64[n+1], a_start i32[n], a_end i32[n], barcode i32[n]) on device,
        bit-identical to synth.generate_packed()."""
        torch = self.torch
        key = (spec.seed, spec.n_barcodes)
        if key not in self._synth_tables:
            lead, bc, dt = spec.tables()
            self._synth_tables[key] = (
                torch.from_numpy(lead).to(self.tdev), torch.from_numpy(bc).to(self.tdev),
                torch.from_numpy(dt).to(self.tdev))
        lead, bc, dt = self._synth_tables[key]
        lens = torch.empty(n_reads, dtype=torch.int64, device=self.tdev)
        _lib.check(self.L.wdx_synth_lengths_dev(self.ctx.handle, spec.seed, first_read, n_reads,
                                                spec.n_barcodes, _dp(dt), _dp(lens), self._stream()))
        off = torch.zeros(n_reads + 1, dtype=torch.int64, device=self.tdev)
        torch.cumsum(lens, 0, out=off[1:])
        total = int(off[-1].item())
        sig = torch.empty(total, dtype=torch.float32, device=self.tdev)
        barcode = torch.empty(n_reads, dtype=torch.int32, device=self.tdev)
        _lib.check(self.L.wdx_synth_fill_dev(
            self.ctx.handle, spec.seed, first_read, n_reads, spec.n_barcodes, spec.n_bc_events,
            float(spec.noise_scale), int(spec.spikes), _dp(dt), _dp(lead), _dp(bc), _dp(off), _dp(sig),
            _dp(barcode), self._stream()))
        a_start = torch.full((n_reads,), synth.PAD, dtype=torch.int32, device=self.tdev)
        a_end = (lens - synth.PAD).to(torch.int32)
        return sig, off, a_start, a_end, barcode, int(lens.max().item())

    # -- measurement ----------------------------------------------------------------------------------
    def kernel_timing(self, enable: bool):
        _lib.check(self.L.wdx_kernel_timing(self.ctx.handle, int(enable)))

    def kernel_time_reset(self):
        _lib.check(self.L.wdx_kernel_time_reset(self.ctx.handle))

    def kernel_time(self, kernel_id: int):
        ms = C.c_double(0)
        n = C.c_int64(0)
        _lib.check(self.L.wdx_kernel_time(self.ctx.handle, kernel_id, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        self.ctx.close()
