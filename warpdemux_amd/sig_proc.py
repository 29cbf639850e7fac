"""MI355X batched counterpart of ``warpdemux.sig_proc.detect_results_to_fpt``.

The reference fingerprints one read per Python call (sig_proc.py:394-605) from a loop over the
minibatch (file_proc.py:418-428).  Here the whole minibatch goes to the HIP engine in one call
(`detect_results_to_fpt_batch`), and thin shims rebuild per-read `ReadResult` objects with the
reference's field names and fail-reason strings so the callers' savers see the same records.

Both branches of the reference are covered: the plain one (``segmentation.consensus_refinement = false``, the
shipped RNA004 config) and the consensus-guided barcode refinement of the tRNA models (sig_proc.py:257-378,
452-521; `RefineParams`, `fingerprint_refine_batch`).  ``refinement_optimal_cpts`` (ruptures KernelCPD, false
in every shipped config) is served behind an option of its own: ``RefineParams.optimal_cpts`` / ``from_spc(...,
optimal_cpts=True)`` -- the stated float64 rule of include/wdx.h; parity with ruptures itself is unpinned.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _lib, _marshal

MAX_ADAPTER_SAMPLES = 16384   # WDX_MAX_ADAPTER_SAMPLES (include/wdx.h)
MAX_LONG_ADAPTER_SAMPLES = 65536   # WDX_MAX_LONG_ADAPTER_SAMPLES: with ``long_windows=True`` (WDX_OPT_LONG_WINDOWS)

# status code -> ReadResult.fail_reason (reference strings: sig_proc.py:400-407, 440-446, 538-544,
# 554-560; file_proc.py:224).  Codes 2 and 4 carry the exception text in the reference; the only
# exception reachable there is mean/mad_normalize's ValueError("Signal contains NaN values.").
FAIL_REASONS = {
    0: "",
    1: None,  # passthrough of detect_results.fail_reason
    2: "signal normalization failed: Signal contains NaN values.",
    3: "event segmentation failed",
    4: "segment normalization failed: Signal contains NaN values.",
    5: "unknown",
    6: "consensus query outlier",
}


@dataclass
class SegParams:
    """Hot-path knobs of SigProcConfig (config/sig_proc.py:16-70); defaults = shipped
    rna004_130bps@v1.0.toml, outlier threshold = ADAPTed's core.sig_norm_outlier_thresh default."""

    padding: int = 100
    sig_norm: str = "none"
    outlier_thresh: float = 5.0
    min_obs_per_base: int = 6
    running_stat_width: int = 12
    num_events: int = 110
    accept_less_cpts: bool = False
    seg_norm: str = "mean"
    barcode_num_events: int = 25
    # evaluation of the clip bounds `med -/+ thresh*mad` (sig_proc.py:426-431), the one NumPy-version-dependent
    # step of the path: "float32" (NumPy >= 2 with a Python-float threshold), "float64" (NumPy 1.x -- the
    # reference pins 1.26.4 -- or an np.float64 threshold), "auto" = the rule of the NumPy this process runs,
    # i.e. what the reference would compute here
    clip_bounds: str = "auto"

    @classmethod
    def from_spc(cls, spc, long_windows: bool = False) -> "SegParams":
        """From a reference-style SigProcConfig (attribute access as in sig_proc.py:414-534).  ``long_windows``: the
        configuration is meant for objects and calls with ``long_windows=True``, which take adapter windows of up to
        WDX_MAX_LONG_ADAPTER_SAMPLES = 65 536 samples (plain and consensus-refinement branch)."""
        seg = spc.segmentation
        k = seg.barcode_num_events
        if getattr(seg, "consensus_refinement", False):
            if isinstance(k, (int, np.integer)):
                # sig_proc.py:455-459
                raise ValueError("barcode_num_events is an integer in consensus refinement mode, use a tuple instead")
            k = int(k[1])
        elif not isinstance(k, (int, np.integer)):
            raise ValueError("barcode_num_events must be an int outside consensus refinement mode")
        # The engine takes adapter windows of at most WDX_MAX_ADAPTER_SAMPLES = 16 384 samples (the shipped configs admit
        # max_obs_trace + 2 * padding = 10 200 / 15 200); the reference has no such limit (sig_proc.py:382-391).  A
        # configuration that admits longer windows (`--export core.max_obs_trace=...`) is refused HERE, once, instead of
        # every such read coming back "unknown" from the kernels.  With ``long_windows`` the limit is
        # WDX_MAX_LONG_ADAPTER_SAMPLES = 65 536.
        mot = getattr(getattr(spc, "core", None), "max_obs_trace", None)
        limit, limit_name = ((MAX_LONG_ADAPTER_SAMPLES, "WDX_MAX_LONG_ADAPTER_SAMPLES") if long_windows else
                             (MAX_ADAPTER_SAMPLES, "WDX_MAX_ADAPTER_SAMPLES"))
        if isinstance(mot, (int, np.integer)) and int(mot) + 2 * int(spc.sig_extract.padding) > limit:
            raise NotImplementedError(
                f"core.max_obs_trace = {int(mot)} with padding {int(spc.sig_extract.padding)} admits adapter windows of "
                f"{int(mot) + 2 * int(spc.sig_extract.padding)} samples; the HIP engine takes at most {limit} "
                f"({limit_name})")
        return cls(
            padding=int(spc.sig_extract.padding),
            sig_norm=str(spc.sig_extract.normalization),
            outlier_thresh=(spc.core.sig_norm_outlier_thresh if isinstance(spc.core.sig_norm_outlier_thresh, np.float64)
                            else float(spc.core.sig_norm_outlier_thresh)),
            min_obs_per_base=int(seg.min_obs_per_base),
            running_stat_width=int(seg.running_stat_width),
            num_events=int(seg.num_events),
            accept_less_cpts=bool(seg.accept_less_cpts),
            seg_norm=str(seg.normalization),
            barcode_num_events=int(k),
        )

    def to_c(self) -> _lib.SegParamsC:
        for name in (self.sig_norm, self.seg_norm):
            if name not in _lib.NORM_CODES:
                msg = f"Normalization method {name} not recognized."
                raise ValueError(msg)
        if self.clip_bounds not in ("auto", "float32", "float64"):
            raise ValueError("clip_bounds must be 'auto', 'float32' or 'float64'")
        f64 = (self.clip_bounds == "float64" or
               (self.clip_bounds == "auto" and (isinstance(self.outlier_thresh, np.float64)
                                                or int(np.__version__.split(".")[0]) < 2)))
        return _lib.SegParamsC(
            self.padding, _lib.NORM_CODES[self.sig_norm], float(self.outlier_thresh), self.min_obs_per_base,
            self.running_stat_width, self.num_events, int(self.accept_less_cpts),
            _lib.NORM_CODES[self.seg_norm], self.barcode_num_events, int(f64), float(self.outlier_thresh),
        )


@dataclass
class RefineParams:
    """segmentation.consensus_* knobs of the refinement branch (config/sig_proc.py:57-66) + the consensus query
    (``warpdemux._consensus.ALL[segmentation.consensus_model]``, passed in by the caller like the reference's
    ``detect_results_to_fpt(..., consensus_query)``)."""

    query: np.ndarray = None
    subseq_norm: str = "mean"
    penalty: float = 1.5
    psi: tuple = (5, 0, 40, 0)
    ub_start: int = 18
    lb_end: int = 69
    ub_end: int = 97
    barcode_segm_events: int = 25
    barcode_keep_events: int = 25
    # segmentation.refinement_optimal_cpts: the barcode tail is cut at its least-squares optimal change-points instead of its
    # strongest peaks (WDX_OPT_REFINE_OPTIMAL_CPTS on the context of the call; not a field of wdx_refine_params)
    optimal_cpts: bool = False

    @classmethod
    def from_spc(cls, spc, consensus_query, optimal_cpts: bool = False) -> "RefineParams":
        """``optimal_cpts=True`` accepts a configuration with ``refinement_optimal_cpts`` (the field is then set from the
        configuration); without the keyword such a configuration is refused, as it always was."""
        seg = spc.segmentation
        if getattr(seg, "refinement_optimal_cpts", False) and not optimal_cpts:
            raise NotImplementedError("refinement_optimal_cpts (ruptures KernelCPD) is not offered by the HIP engine")
        k = seg.barcode_num_events
        if isinstance(k, (int, np.integer)):
            raise ValueError("barcode_num_events is an integer in consensus refinement mode, use a tuple instead")
        if not isinstance(k, (tuple, list, np.ndarray)):
            raise TypeError("barcode_num_events must be a tuple, list or numpy array when using multiple values")
        q = np.ascontiguousarray(consensus_query, dtype=np.float64)
        if q.ndim != 1 or q.size == 0:
            raise ValueError("consensus refinement needs a 1-D consensus query")
        return cls(query=q, subseq_norm=str(seg.consensus_subseq_match_normalization),
                   penalty=float(seg.consensus_subseq_match_penalty),
                   psi=tuple(int(v) for v in seg.consensus_subseq_match_psi),
                   ub_start=int(seg.consensus_subseq_match_ub_start), lb_end=int(seg.consensus_subseq_match_lb_end),
                   ub_end=int(seg.consensus_subseq_match_ub_end), barcode_segm_events=int(k[0]),
                   barcode_keep_events=int(k[1]),
                   optimal_cpts=bool(optimal_cpts and getattr(seg, "refinement_optimal_cpts", False)))

    def to_c(self) -> "_lib.RefineParamsC":
        if self.subseq_norm not in _lib.NORM_CODES:
            raise ValueError(f"Normalization method {self.subseq_norm} not recognized.")
        self._q = np.ascontiguousarray(self.query, dtype=np.float64)   # kept alive with the object
        return _lib.RefineParamsC(self._q.ctypes.data, int(self._q.size), _lib.NORM_CODES[self.subseq_norm],
                                  float(self.penalty), (C.c_int32 * 4)(*[int(v) for v in self.psi]), self.ub_start,
                                  self.lb_end, self.ub_end, self.barcode_segm_events, self.barcode_keep_events)


@dataclass
class DetectResults:
    """The four fields of ADAPTed's DetectResults the hot path reads (sig_proc.py:400-418)."""

    success: bool = True
    fail_reason: str = ""
    adapter_start: Optional[int] = None
    adapter_end: Optional[int] = None


# WDX_DETECT_* code -> DetectResults.fail_reason.  The strings are the engine's own, like the rule (include/wdx.h: the engine's
# own rule; parity with ADAPTed unpinned; accuracy on real reads unmeasured).
DETECT_FAIL_REASONS = {
    0: "",
    1: "trace too short for an adapter and a polyA window",
    2: "no adapter start below the open-pore level",
    3: "no room for an adapter end behind the start",
    4: "no polyA-like window behind the adapter",
}


@dataclass
class DetectParams:
    """wdx_detect_params (include/wdx.h states the rule bit for bit and the domain): the engine's own boundary detection ahead of
    every entry that takes ``a_start`` / ``a_end`` / ``ok``.  The defaults are the values the rule was prototyped with on
    synthetic RNA004-like traces; accuracy on real reads is unmeasured."""

    max_obs_trace: int = 10000
    quant_per_pa: float = 8.0
    find_start: bool = True
    open_pore_pa: float = 150.0
    start_win: int = 32
    max_start: int = 2000
    min_obs_adapter: int = 1000
    max_obs_adapter: int = 8000
    polya_win: int = 200
    step_win: int = 8
    refine: int = 300
    min_shift_pa: float = 8.0
    max_polya_var: float = 9.0

    def to_c(self) -> "_lib.DetectParamsC":
        """The C structure, after the domain check the library makes too (``ValueError``)."""
        ints = ("max_obs_trace", "start_win", "max_start", "min_obs_adapter", "max_obs_adapter", "polya_win", "step_win", "refine")
        for name in ints:
            v = getattr(self, name)
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not -2**31 <= int(v) < 2**31:
                raise ValueError(f"DetectParams.{name} must be an int32")
        with np.errstate(over="ignore"):   # (a value beyond float32 becomes infinite and is refused below)
            floats = [np.float32(getattr(self, name)) for name in ("quant_per_pa", "open_pore_pa", "min_shift_pa", "max_polya_var")]
        if not all(np.isfinite(f) for f in floats):
            raise ValueError("DetectParams: quant_per_pa, open_pore_pa, min_shift_pa and max_polya_var must be finite float32")
        if not 1 <= self.max_obs_trace <= _lib.DETECT_MAX_TRACE:
            raise ValueError(f"DetectParams.max_obs_trace = {self.max_obs_trace} (1..{_lib.DETECT_MAX_TRACE})")
        if not floats[0] > 0:
            raise ValueError(f"DetectParams.quant_per_pa = {self.quant_per_pa} must be positive")
        if self.find_start not in (0, 1):
            raise ValueError("DetectParams.find_start is 0 / 1")
        if not 1 <= self.step_win <= self.polya_win <= 1024:
            raise ValueError("DetectParams: 1 <= step_win <= polya_win <= 1024")
        if not self.step_win <= self.min_obs_adapter <= self.max_obs_adapter:
            raise ValueError("DetectParams: step_win <= min_obs_adapter <= max_obs_adapter")
        if not 1 <= self.start_win <= 256:
            raise ValueError("DetectParams: 1 <= start_win <= 256")
        if not 0 <= self.refine <= 4096:
            raise ValueError("DetectParams: 0 <= refine <= 4096")
        if self.max_start < 0:
            raise ValueError("DetectParams.max_start must not be negative")
        return _lib.DetectParamsC(int(self.max_obs_trace), float(floats[0]), int(self.find_start), float(floats[1]),
                                  int(self.start_win), int(self.max_start), int(self.min_obs_adapter), int(self.max_obs_adapter),
                                  int(self.polya_win), int(self.step_win), int(self.refine), float(floats[2]), float(floats[3]))


@dataclass
class DetectBatch:
    """Struct-of-arrays result of the boundary detection on one minibatch (include/wdx.h: the outputs per read)."""

    a_start: np.ndarray   # (n,) int32, -1 where no start was found
    a_end: np.ndarray     # (n,) int32, -1 unless the read succeeded
    ok: np.ndarray        # (n,) uint8
    code: np.ndarray      # (n,) int32 WDX_DETECT_*
    info: np.ndarray      # (n, 4) int32 {n, c, P[e] - P[s], P[e + polya_win] - P[e]}
    gain: np.ndarray      # (n,) float64 g(c)

    def results(self) -> List["DetectResults"]:
        """one `DetectResults` per read, as the fingerprint shims take them"""
        return [DetectResults(success=bool(self.ok[i]), fail_reason=DETECT_FAIL_REASONS[int(self.code[i])],
                              adapter_start=int(self.a_start[i]) if self.a_start[i] >= 0 else None,
                              adapter_end=int(self.a_end[i]) if self.a_end[i] >= 0 else None) for i in range(len(self.code))]


def _detect_outputs(n):
    return DetectBatch(np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint8), np.empty(n, np.int32),
                       np.empty((n, 4), np.int32), np.empty(n, np.float64))


def _detect_row_len(row_len, n, stride, required):
    if row_len is None:
        if required:
            raise ValueError("row_len is required for int16 rows (there is no NaN tail to find the end by)")
        return None
    row_len = np.ascontiguousarray(row_len, dtype=np.int32)
    if row_len.shape != (n,):
        raise ValueError("row_len must have one entry per read")
    return row_len


def detect_batch_arrays(signals, params: Optional[DetectParams] = None, row_len=None, device=None) -> DetectBatch:
    """Boundary detection on a (n_reads, stride) float32 minibatch with a NaN tail (wdx_detect_batch): the arrays."""
    sig = np.ascontiguousarray(signals, dtype=np.float32)
    if sig.ndim != 2:
        raise ValueError("signals must be a 2-D (n_reads, stride) array")
    n, stride = sig.shape
    pc = (params or DetectParams()).to_c()
    row_len = _detect_row_len(row_len, n, stride, False)
    o = _detect_outputs(n)
    _lib.check(_lib.load().wdx_detect_batch(
        _lib.default_context(device).handle, _lib.ptr(sig), n, stride, _lib.ptr(row_len), C.byref(pc), _lib.ptr(o.a_start),
        _lib.ptr(o.a_end), _lib.ptr(o.ok), _lib.ptr(o.code), _lib.ptr(o.info), _lib.ptr(o.gain)))
    return o


def detect_batch(signals, params: Optional[DetectParams] = None, row_len=None, device=None) -> List[DetectResults]:
    """The module-level, host-fed boundary detection: one `DetectResults` per row of a (n_reads, stride) float32 minibatch --
    what `detect_results_to_fpt_batch` takes.  The engine's own rule; parity with ADAPTed unpinned; accuracy on real reads
    unmeasured."""
    return detect_batch_arrays(signals, params, row_len, device).results()


def detect_batch_adc(adc, row_len, offset, scale, params: Optional[DetectParams] = None, device=None) -> DetectBatch:
    """`detect_batch_arrays` for a (n_reads, stride) int16 ADC minibatch (wdx_detect_batch_adc); bit-identical to it on
    ``calibrate_adc(adc, row_len, offset, scale)``."""
    adc = np.asarray(adc)
    if adc.ndim != 2 or adc.dtype != np.int16 or not adc.flags.c_contiguous:
        raise ValueError("adc must be a C-contiguous 2-D (n_reads, stride) int16 array")
    n, stride = adc.shape
    row_len = _detect_row_len(row_len, n, stride, True)
    off, sc = np.ascontiguousarray(offset, dtype=np.float32), np.ascontiguousarray(scale, dtype=np.float32)
    if off.shape != (n,) or sc.shape != (n,):
        raise ValueError("offset and scale must have one entry per read")
    pc = (params or DetectParams()).to_c()
    o = _detect_outputs(n)
    _lib.check(_lib.load().wdx_detect_batch_adc(
        _lib.default_context(device).handle, _lib.ptr(adc), n, stride, _lib.ptr(row_len), _lib.ptr(off), _lib.ptr(sc), C.byref(pc),
        _lib.ptr(o.a_start), _lib.ptr(o.a_end), _lib.ptr(o.ok), _lib.ptr(o.code), _lib.ptr(o.info), _lib.ptr(o.gain)))
    return o


@dataclass
class ReadResult:
    """Same fields as warpdemux.sig_proc.ReadResult (sig_proc.py:26-62)."""

    read_id: Optional[str] = None
    success: bool = True
    fail_reason: str = ""
    detect_results: Any = None
    barcode_fpt: Optional[np.ndarray] = None
    dwell_times: Optional[np.ndarray] = None
    adapter_dt_med: Optional[float] = None
    adapter_dt_mad: Optional[float] = None
    adapter_event_mean: Optional[float] = None
    adapter_event_std: Optional[float] = None
    adapter_event_med: Optional[float] = None
    adapter_event_mad: Optional[float] = None
    seg_cons_query_start: Optional[int] = None
    seg_cons_query_end: Optional[int] = None
    sig_barcode_start: Optional[int] = None

    def to_summary_dict(self) -> Dict[str, Any]:
        return {
            "read_id": self.read_id,
            "success": self.success,
            "fail_reason": self.fail_reason,
            "adapter_dt_med": self.adapter_dt_med,
            "adapter_dt_mad": self.adapter_dt_mad,
            "adapter_event_mean": self.adapter_event_mean,
            "adapter_event_std": self.adapter_event_std,
            "adapter_event_med": self.adapter_event_med,
            "adapter_event_mad": self.adapter_event_mad,
            "seg_cons_query_start": self.seg_cons_query_start,
            "seg_cons_query_end": self.seg_cons_query_end,
            "sig_barcode_start": self.sig_barcode_start,
        }

    def set_read_id(self, read_id: str):
        self.read_id = read_id


@dataclass
class FingerprintBatch:
    """Struct-of-arrays result of one minibatch."""

    fpt: np.ndarray      # (n, K) float64, NaN rows for failed reads
    dwell: np.ndarray    # (n, K) int64
    stats: np.ndarray    # (n, 6) float64: dt_med, dt_mad, event_mean, event_std, event_med, event_mad
    status: np.ndarray   # (n,) int32, WDX_READ_*
    refine_idx: Optional[np.ndarray] = None   # (n, 3) int32 seg_cons_query_start / _end, sig_barcode_start (refinement)

    @property
    def success(self) -> np.ndarray:
        return self.status == 0


_FPT_WANT = _lib.WANT_FPT | _lib.WANT_DWELL | _lib.WANT_STATS    # the ReadResult arrays of a minibatch


def fingerprints(o: dict) -> FingerprintBatch:
    """`FingerprintBatch` of a minibatch's result arrays (`_marshal.outputs`)"""
    return FingerprintBatch(o["fpt"], o["dwell"], o["stats"], o["status"], o["refine_idx"])


def fingerprint_batch(signals, adapter_start, adapter_end, params: SegParams, success=None, device=None,
                      long_windows: bool = False) -> FingerprintBatch:
    """Fingerprint a (n_reads, stride) float32 minibatch (file_proc.py:244-260 layout, NaN tail).  ``long_windows``:
    adapter windows of up to MAX_LONG_ADAPTER_SAMPLES samples for this call (WDX_OPT_LONG_WINDOWS on the default context,
    put back afterwards); the default reports windows beyond MAX_ADAPTER_SAMPLES as failed ("unknown")."""
    sig, a_s, a_e, ok, n, stride = _marshal.minibatch(signals, adapter_start, adapter_end, success)
    pc = params.to_c()
    o = _marshal.outputs(n, params.barcode_num_events, 0, 0, _FPT_WANT)
    with _lib.default_context(device).long_windows_for_call(long_windows) as ctx:
        _lib.check(_lib.load().wdx_fingerprint_batch(
            ctx.handle, _lib.ptr(sig), n, stride, _lib.ptr(a_s), _lib.ptr(a_e), _lib.ptr(ok), C.byref(pc), _lib.ptr(o["fpt"]),
            _lib.ptr(o["dwell"]), _lib.ptr(o["stats"]), _lib.ptr(o["status"])))
    return fingerprints(o)


def calibrate_adc(adc, row_len, offset, scale, stride=None) -> np.ndarray:
    """THE CONTRACT of the int16 way in, in NumPy: the float32 minibatch the ``*_adc`` entry points stand for.

    Row r holds ``scale[r] * (float32(adc[r, i]) + offset[r])`` for ``i < row_len[r]`` -- a float32 add, then a float32
    multiply: two roundings, never one fused operation -- and NaN from there to ``stride`` (the NaN tail of
    file_proc.py:255-260).  Every ``*_adc`` call returns, bit for bit, what its float32 counterpart returns on this array.
    A reader that calibrates by another formula (another order of operations, float64 arithmetic) is not served by the
    int16 path: compare its rows with this function's first.

    The same array is what an int16 shard that stays in device memory stands for: ``engine.AdcShard`` (the ``*_adc_dev``
    entry points), accepted by every ``DemuxEngine`` method that takes ``sig`` -- a packed shard's row ends at ``row_win``
    instead of ``stride``.  The same caveat applies there."""
    adc = np.asarray(adc)
    if adc.ndim != 2 or adc.dtype != np.int16:
        raise ValueError("adc must be a 2-D (n_reads, stride) int16 array")
    n, width = adc.shape
    stride = width if stride is None else int(stride)
    if stride < width:
        raise ValueError("stride must not be smaller than the rows of adc")
    row_len = np.asarray(row_len, dtype=np.int64)
    off = np.asarray(offset, dtype=np.float32)
    sc = np.asarray(scale, dtype=np.float32)
    if row_len.shape != (n,) or off.shape != (n,) or sc.shape != (n,):
        raise ValueError("row_len, offset and scale must have one entry per read")
    if n and (row_len.min() < 0 or row_len.max() > width):
        raise ValueError("row_len must be within 0 .. the rows of adc")
    out = np.full((n, stride), np.nan, dtype=np.float32)
    summed = adc.astype(np.float32) + off[:, None]     # float32 + float32 -> float32, rounded once
    np.multiply(summed, sc[:, None], out=summed)       # ... and once more
    live = np.arange(width)[None, :] < row_len[:, None]
    out[:, :width][live] = summed[live]
    return out


def adc_minibatch(adc, row_len, offset, scale, adapter_start, adapter_end, success=None, row_off=None, row_win=None):
    """Check an int16 minibatch before anything of it is passed by address -- shapes and dtypes of every array,
    ``success`` included -- and lay it out as `_lib.MinibatchAdcInC`.  Returns ``(descriptor, n_reads, kept)``; `kept`
    holds the arrays the descriptor points into.  ``adc`` itself is never copied or converted: an array that is not
    C-contiguous int16 is refused (the point of this path is the bytes that do not move).

    ``row_off`` (int64[n + 1], multiples of 8): `adc` is 1-D and holds packed rows, row r = its ``row_len[r]`` samples at
    ``adc[row_off[r]:]``, adapter bounds relative to the row; ``row_win`` (optional) = samples of the float32 row it
    stands for, the surplus over ``row_len`` being NaN tail."""
    a, n, stride, *rest = _marshal.adc_rows(adc, row_len, offset, scale, adapter_start, adapter_end, success, row_off, row_win)
    kept = (a, *rest)     # adc, row_len, offset, scale, row_off, row_win, a_start, a_end, ok: the descriptor's pointers, in order
    desc = _lib.MinibatchAdcInC(_lib.addr(a), n, stride, *[_lib.addr(v) for v in rest])
    return desc, n, kept


def fingerprint_batch_adc(adc, row_len, offset, scale, adapter_start, adapter_end, params: SegParams, success=None,
                          device=None, long_windows: bool = False) -> FingerprintBatch:
    """`fingerprint_batch` for a (n_reads, stride) int16 ADC minibatch: 2 bytes per sample over the bus, calibrated on the
    device.  Bit-identical to ``fingerprint_batch(calibrate_adc(adc, row_len, offset, scale), ...)``."""
    desc, n, kept = adc_minibatch(adc, row_len, offset, scale, adapter_start, adapter_end, success)
    pc = params.to_c()
    o = _marshal.outputs(n, params.barcode_num_events, 0, 0, _FPT_WANT)
    with _lib.default_context(device).long_windows_for_call(long_windows) as ctx:
        _lib.check(_lib.load().wdx_fingerprint_batch_adc(ctx.handle, C.byref(desc), C.byref(pc), _lib.ptr(o["fpt"]),
                                                         _lib.ptr(o["dwell"]), _lib.ptr(o["stats"]), _lib.ptr(o["status"])))
    del kept
    return fingerprints(o)


def fingerprint_refine_batch(signals, adapter_start, adapter_end, params: SegParams, refine: RefineParams, success=None,
                             device=None, long_windows: bool = False) -> FingerprintBatch:
    """Consensus-refinement branch on a (n_reads, stride) float32 minibatch; K = refine.barcode_keep_events.
    ``long_windows``: adapter windows of up to MAX_LONG_ADAPTER_SAMPLES samples for this call (WDX_OPT_LONG_REFINE_WINDOWS on
    the default context, put back afterwards); the default reports windows beyond MAX_ADAPTER_SAMPLES as failed ("unknown").
    ``refine.optimal_cpts``: WDX_OPT_REFINE_OPTIMAL_CPTS for this call, in the same way; not together with ``long_windows``."""
    _marshal.refine_options(refine, long_windows, "fingerprint_refine_batch")
    sig, a_s, a_e, ok, n, stride = _marshal.minibatch(signals, adapter_start, adapter_end, success)
    pc, rc = params.to_c(), refine.to_c()
    o = _marshal.outputs(n, refine.barcode_keep_events, 0, 0, _FPT_WANT | _lib.WANT_REFINE_IDX)
    with _lib.default_context(device).refine_options_for_call(refine, long_windows) as ctx:
        _lib.check(_lib.load().wdx_fingerprint_refine_batch(
            ctx.handle, _lib.ptr(sig), n, stride, _lib.ptr(a_s), _lib.ptr(a_e), _lib.ptr(ok), C.byref(pc), C.byref(rc),
            _lib.ptr(o["fpt"]), _lib.ptr(o["dwell"]), _lib.ptr(o["stats"]), _lib.ptr(o["refine_idx"]), _lib.ptr(o["status"])))
    return fingerprints(o)


@dataclass
class DemuxBatch:
    """Result of the fused host call: fingerprint -> DTW -> nearest reference."""

    status: np.ndarray            # (n,) int32 WDX_READ_*
    call: np.ndarray              # (n,) int32 argmin reference index, -1 for failed reads
    dist: Optional[np.ndarray]    # (n, nY) float32, NaN rows for failed reads
    fpt: Optional[np.ndarray]     # (n, K) float64


def set_references(refs, window=None, penalty=None, device=None):
    """Upload the reference set once (model._X) for `demux_batch`; kept resident in the context."""
    refs = np.ascontiguousarray(refs, dtype=np.float64)
    if refs.ndim != 2:
        raise ValueError("refs must be (nY, L)")
    ctx = _lib.default_context(device)
    _submit_references(ctx, refs, window, penalty)
    ctx._demux_refs = (refs, window, penalty)   # re-submitted by demux_batch if another call replaces them
    return refs.shape


def _submit_references(ctx, refs, window, penalty):
    _marshal.set_refs(ctx, refs, window, penalty)
    gen = C.c_int64(0)
    _lib.check(_lib.load().wdx_refs_generation(ctx.handle, C.byref(gen)))
    ctx._demux_refs_gen = gen.value


def _held_references(ctx, who: str, n_refs=None) -> int:
    """How many references `set_references` installed in this context, after making sure they are still the resident set:
    distance_matrix_to / a DTW_SVM model may have replaced it, and one counter read per call tells (wdx_refs_generation).  The
    distance matrix is sized from this number, never from the caller (the C ABI checks it against the resident set once
    more)."""
    held = getattr(ctx, "_demux_refs", None)
    if held is None:
        raise _lib.WdxError(f"{who}: no reference set -- call set_references() first")
    n_held = int(held[0].shape[0])
    if n_refs is not None and int(n_refs) != n_held:
        raise ValueError(f"n_refs={n_refs} but set_references() installed {n_held} references")
    gen = C.c_int64(0)
    _lib.check(_lib.load().wdx_refs_generation(ctx.handle, C.byref(gen)))
    if gen.value != ctx._demux_refs_gen:
        _submit_references(ctx, *held)
    return n_held


def _demux_want(want_dist, want_fpt) -> int:
    return (_lib.WANT_DIST if want_dist else 0) | (_lib.WANT_FPT if want_fpt else 0)


def demux_batch(signals, adapter_start, adapter_end, params: SegParams, success=None, want_dist=True,
                want_fpt=False, n_refs=None, device=None, long_windows: bool = False) -> DemuxBatch:
    """One call per minibatch / live tick: fingerprints, distances to the resident references
    (`set_references`) and the nearest-reference call, with a single device synchronisation."""
    sig, a_s, a_e, ok, n, stride = _marshal.minibatch(signals, adapter_start, adapter_end, success)
    pc = params.to_c()
    ctx = _lib.default_context(device)
    n_held = _held_references(ctx, "demux_batch", n_refs)
    o = _marshal.outputs(n, params.barcode_num_events, n_held, 0, _demux_want(want_dist, want_fpt))
    with ctx.long_windows_for_call(long_windows):
        _lib.check(_lib.load().wdx_demux_batch(
            ctx.handle, _lib.ptr(sig), n, stride, _lib.ptr(a_s), _lib.ptr(a_e), _lib.ptr(ok), C.byref(pc),
            n_held, _lib.ptr(o["fpt"]), _lib.ptr(o["dist"]), _lib.ptr(o["call"]), _lib.ptr(o["status"])))
    return DemuxBatch(o["status"], o["call"], o["dist"], o["fpt"])


def demux_batch_adc(adc, row_len, offset, scale, adapter_start, adapter_end, params: SegParams, success=None, want_dist=True,
                    want_fpt=False, device=None, long_windows: bool = False) -> DemuxBatch:
    """`demux_batch` for a (n_reads, stride) int16 ADC minibatch (wdx_demux_batch_adc); bit-identical to `demux_batch` on
    ``calibrate_adc(adc, row_len, offset, scale)``."""
    desc, n, kept = adc_minibatch(adc, row_len, offset, scale, adapter_start, adapter_end, success)
    pc = params.to_c()
    ctx = _lib.default_context(device)
    n_held = _held_references(ctx, "demux_batch_adc")
    o = _marshal.outputs(n, params.barcode_num_events, n_held, 0, _demux_want(want_dist, want_fpt))
    with ctx.long_windows_for_call(long_windows):
        _lib.check(_lib.load().wdx_demux_batch_adc(ctx.handle, C.byref(desc), C.byref(pc), n_held, _lib.ptr(o["fpt"]),
                                                   _lib.ptr(o["dist"]), _lib.ptr(o["call"]), _lib.ptr(o["status"])))
    del kept
    return DemuxBatch(o["status"], o["call"], o["dist"], o["fpt"])


def detect_results_to_fpt_batch(calibrated_signals, spc, detect_results: Sequence, read_ids: Optional[Sequence[str]] = None,
                                device=None, consensus_query=None, long_windows: bool = False,
                                optimal_cpts: bool = False) -> List[ReadResult]:
    """Batched `detect_results_to_fpt`: one ReadResult per row, identical fields to the reference's
    per-read call (sig_proc.py:590-605) plus the `barcode_fpt_wrapper` read-id (file_proc.py:216).  With
    ``spc.segmentation.consensus_refinement`` the caller passes the consensus signal like the reference does.
    ``long_windows``: a configuration with ``core.max_obs_trace`` + 2 x padding up to MAX_LONG_ADAPTER_SAMPLES is accepted and
    its long windows are fingerprinted, on the plain and on the consensus-refinement branch.  ``optimal_cpts``: a configuration
    with ``segmentation.refinement_optimal_cpts`` is accepted and served (`RefineParams.from_spc`); refused without it."""
    params = SegParams.from_spc(spc, long_windows=long_windows)
    refine = None
    if getattr(spc.segmentation, "consensus_refinement", False):
        if consensus_query is None or np.asarray(consensus_query).size == 0:
            raise ValueError("consensus_model must be specified when consensus_refinement is True")
        refine = RefineParams.from_spc(spc, consensus_query, **(dict(optimal_cpts=True) if optimal_cpts else {}))
    n = len(detect_results)
    ok = np.array([bool(d.success) for d in detect_results], dtype=np.uint8)
    a_s = np.array([d.adapter_start if (d.success and d.adapter_start is not None) else 0 for d in detect_results], dtype=np.int32)
    a_e = np.array([d.adapter_end if (d.success and d.adapter_end is not None) else 0 for d in detect_results], dtype=np.int32)
    if refine is None:
        fb = fingerprint_batch(calibrated_signals, a_s, a_e, params, success=ok, device=device, long_windows=long_windows)
    else:
        kw = dict(long_windows=True) if long_windows else {}     # (the default call is what it has always been)
        fb = fingerprint_refine_batch(calibrated_signals, a_s, a_e, params, refine, success=ok, device=device, **kw)
    return read_results_from_batch(fb, detect_results, read_ids, refined=refine is not None)


def read_results_from_batch(fb: FingerprintBatch, detect_results: Sequence, read_ids: Optional[Sequence[str]] = None,
                            refined: bool = False) -> List[ReadResult]:
    """The per-read ``ReadResult`` records of one fingerprinted minibatch (sig_proc.py:590-605 + the read id of
    ``barcode_fpt_wrapper``, file_proc.py:216) -- shared by `detect_results_to_fpt_batch` and the feeder's workers."""
    n = len(detect_results)
    out = []
    for i in range(n):
        st = int(fb.status[i])
        rid = None if read_ids is None else read_ids[i]
        extra = {}
        if refined and st in (0, 6):
            q = fb.refine_idx[i]
            extra = dict(seg_cons_query_start=int(q[0]), seg_cons_query_end=int(q[1]), sig_barcode_start=int(q[2]))
        if st == 0 or st == 6:
            s = fb.stats[i]
            out.append(ReadResult(
                read_id=rid, success=st == 0, fail_reason=FAIL_REASONS[st], detect_results=detect_results[i],
                barcode_fpt=fb.fpt[i].copy() if st == 0 else np.array([]),
                dwell_times=fb.dwell[i].copy() if st == 0 else np.array([]),
                adapter_dt_med=float(s[0]), adapter_dt_mad=float(s[1]), adapter_event_mean=float(s[2]),
                adapter_event_std=float(s[3]), adapter_event_med=float(s[4]), adapter_event_mad=float(s[5]), **extra,
            ))
        elif st == 5:
            # barcode_fpt_wrapper's except-branch builds a bare record (file_proc.py:220-224)
            out.append(ReadResult(read_id=rid, success=False, fail_reason="unknown"))
        else:
            reason = detect_results[i].fail_reason if st == 1 else FAIL_REASONS[st]
            out.append(ReadResult(
                read_id=rid, success=False, fail_reason=reason, detect_results=detect_results[i],
                barcode_fpt=np.array([]), dwell_times=np.array([]),
            ))
    return out


def detect_results_to_fpt(calibrated_signal, spc, detect_results, consensus_query=np.array([]), optimal_cpts: bool = False) -> ReadResult:
    """Per-read signature of the reference (sig_proc.py:394-399); a batch of one."""
    sig = np.asarray(calibrated_signal, dtype=np.float32).reshape(1, -1)
    kw = dict(optimal_cpts=True) if optimal_cpts else {}
    return detect_results_to_fpt_batch(sig, spc, [detect_results], consensus_query=consensus_query, **kw)[0]
