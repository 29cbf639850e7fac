"""Boundary detection on the device (wdx_detect_rows and its kin, include/wdx.h) against the NumPy restatement of the rule
(tests/helpers/detect_rule.py): array_equal on a_start, a_end, ok, code and info, the bits of gain.  The restatement of every
batch is computed once per process and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import detect_rule as dr
from helpers import framed as fr
from helpers import stream_order as so
from warpdemux_amd import _lib, sig_proc

pytestmark = pytest.mark.gpu

FIELDS = ("a_start", "a_end", "ok", "code", "info", "gain")
OUT_SPEC = (("a_start", "int32", 1), ("a_end", "int32", 1), ("ok", "uint8", 1), ("code", "int32", 1), ("info", "int32", 4),
            ("gain", "float64", 1))
SYNTH_SEED = 2024


def _torch():
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def _eng():
    from warpdemux_amd import engine

    refs = np.ascontiguousarray(np.random.default_rng(5).normal(size=(4, 25)))
    return engine.DemuxEngine(refs, 15, 0.1)


def _params(p):
    return sig_proc.DetectParams(**p)


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _host(d):
    """the tensors of a `DetectResult` as NumPy arrays"""
    _torch().cuda.synchronize()
    return {f: getattr(d, f).cpu().numpy() for f in FIELDS}


def _check(got, E, what=""):
    for f in FIELDS:
        want = getattr(E, f)
        g = np.asarray(got[f])
        assert g.dtype == want.dtype and g.shape == want.shape, (what, f, g.dtype, g.shape)
        if f == "gain":
            g, want = g.view(np.int64), want.view(np.int64)
        bad = np.flatnonzero((g != want).reshape(len(want), -1).any(axis=1))
        assert bad.size == 0, "%s %s: %d reads differ, first %d: got %s, want %s" % (what, f, bad.size, bad[0], g[bad[0]], want[bad[0]])


# ---- the shared batches and their restatements ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _small():
    rows, lengths = dr.small_batch(7, 1000)
    return rows, lengths, dr.detect_rows(rows, dr.SMALL)


@functools.lru_cache(maxsize=None)
def _synth(n=512):
    rows, truth = dr.synth_batch(SYNTH_SEED, n)
    return rows, dr.detect_rows(rows, dr.DEFAULT)


@pytest.mark.parametrize("n", [1, 2, 65, 1000])
def test_small_parameters_every_code_and_tie(n):
    rows, lengths, E = _small()
    assert sorted(set(E.code.tolist())) == [0, 1, 2, 3, 4] and E.g_tie.any() and E.d_tie.any()
    assert set(dr.SMALL_LENGTHS) <= set(lengths.tolist())
    eng = _eng()
    eng.kernel_timing(True)
    eng.kernel_time_reset()
    d = eng.detect(_dev(rows[:n]), params=_params(dr.SMALL), want_info=True)
    _check(_host(d), E.take(slice(0, n)), "n=%d" % n)
    ms, launches = eng.kernel_time(_lib.K_DETECT)
    eng.kernel_timing(False)
    assert launches == 1 and ms > 0


def _widen(rows, stride, fill_some):
    out = np.full((rows.shape[0], stride), np.nan, dtype=np.float32)
    out[:, :rows.shape[1]] = rows
    if fill_some:      # every fourth row runs to the end of its stride: no NaN, the cap ends it
        for r in range(0, rows.shape[0], 4):
            n = int(np.flatnonzero(np.isnan(out[r]))[0])
            body = out[r, max(0, n - 700):n].copy()
            reps = -(-(stride - n) // body.size)
            out[r, n:] = np.tile(body, reps)[:stride - n]
    return out


DEFAULT_CASES = {
    "trace10000-stride12000": (dict(max_obs_trace=10000), dr.SYNTH_STRIDE, False),
    "trace16384-stride16384": (dict(max_obs_trace=16384), 16384, True),
    "trace16384-stride16385-no-start": (dict(max_obs_trace=16384, find_start=0), 16385, True),
    "trace10000-stride16385-no-start": (dict(max_obs_trace=10000, find_start=0), 16385, False),
}


@functools.lru_cache(maxsize=None)
def _default_case(name):
    change, stride, fill = DEFAULT_CASES[name]
    rows = _widen(_synth()[0][:256], stride, fill)
    p = dict(dr.DEFAULT, **change)
    return rows, p, dr.detect_rows(rows, p)


@pytest.mark.parametrize("name", list(DEFAULT_CASES))
def test_default_parameters_on_synthetic_traces(name):
    rows, p, E = _default_case(name)
    assert (E.code == dr.OK).mean() > 0.5
    assert (np.isnan(rows[:, :p["max_obs_trace"]]).sum(axis=1) == 0).any()         # rows the cap truncates
    d = _eng().detect(_dev(rows), params=_params(p), want_info=True)
    _check(_host(d), E, name)


@functools.lru_cache(maxsize=None)
def _extremes(find_start, min_shift):
    n = 16384
    half = np.where(np.arange(n) < n // 2, 4095.9, -4095.9)
    saw = np.where((np.arange(n) // 3000) % 2 == 0, -4095.9, 4095.9)
    rows = np.stack([np.full(n, np.inf), np.full(n, -np.inf), np.full(n, 4095.9), np.full(n, -4095.9), np.full(n, 100.0), half, -half,
                     saw]).astype(np.float32)
    p = dict(dr.DEFAULT, max_obs_trace=n, find_start=find_start, min_shift_pa=min_shift)
    return rows, p, dr.detect_rows(rows, p)


@pytest.mark.parametrize("find_start,min_shift", [(0, 0.0), (1, 0.0), (1, 8.0), (0, -100000.0)])
def test_extremes(find_start, min_shift):
    rows, p, E = _extremes(find_start, min_shift)
    if find_start == 0:
        assert E.g_tie[[1, 4]].all() and np.abs(E.info[:, 2].astype(np.int64)).max() >= 1000 * 32767    # the largest sums
    d = _eng().detect(_dev(rows), params=_params(p), want_info=True)
    _check(_host(d), E, "extremes")


CLAMPS = [dict(open_pore_pa=4096.0), dict(open_pore_pa=1e30), dict(open_pore_pa=-4096.0), dict(open_pore_pa=-1e30),
          dict(min_shift_pa=8192.0), dict(min_shift_pa=1e30), dict(min_shift_pa=-8192.0, open_pore_pa=1e30), dict(min_shift_pa=-1e30),
          dict(max_polya_var=1e30, min_shift_pa=-1e30, open_pore_pa=1e30), dict(max_polya_var=33554432.0, min_shift_pa=-1e30),
          dict(max_polya_var=-5.0, min_shift_pa=-1e30), dict(max_polya_var=0.0, min_shift_pa=-1e30)]


@functools.lru_cache(maxsize=None)
def _clamp_case(k):
    p = dict(dr.SMALL, **CLAMPS[k])
    return p, dr.detect_rows(_small()[0][:200], p)


@pytest.mark.parametrize("k", range(len(CLAMPS)), ids=lambda k: "-".join("%s=%g" % kv for kv in CLAMPS[k].items()))
def test_thresholds_at_their_clamps(k):
    """`DetectParams.to_c()`, the library's conversion (thr1, shift_q, var_q with their clamps: include/wdx.h) and the restatement's
    give the same results with a threshold at its clamp value and far beyond it"""
    p, E = _clamp_case(k)
    change = CLAMPS[k]
    if change.get("open_pore_pa", 0) < 0:
        assert not (E.code > dr.NO_START).any()                # q < thr1 never holds
    if change.get("open_pore_pa", 0) > 0:
        assert not (E.code == dr.NO_START).any() and (E.a_start[E.code != dr.SHORT] == 0).all()
    if change.get("min_shift_pa", 0) >= 8192.0 or change.get("max_polya_var", 1) < 0:
        assert not (E.code == dr.OK).any()
    if "max_polya_var" in change and change["max_polya_var"] > 1:
        assert not (E.code == dr.NO_POLYA).any()               # every window is flat enough and high enough
    d = _eng().detect(_dev(_small()[0][:200]), params=_params(p), want_info=True)
    _check(_host(d), E, str(change))


def test_three_layouts_agree():
    rows, lengths, E = _small()
    torch, eng, p = _torch(), _eng(), _params(dr.SMALL)
    n, stride = rows.shape
    a = _host(eng.detect(_dev(rows), params=p, want_info=True))
    junk = np.where(np.isnan(rows), np.float32(77.0), rows)          # no NaN tail: the lengths end the rows
    b = _host(eng.detect(_dev(junk), row_len=_dev(lengths), params=p, want_info=True))
    off = np.concatenate(([0], np.cumsum(lengths.astype(np.int64))))
    packed = np.concatenate([rows[r, :lengths[r]] for r in range(n)])
    c = _host(eng.detect(_dev(packed), offsets=_dev(off), params=p, want_info=True))
    # packed rows with lengths: every other read stops short of its slice
    cut = np.where(np.arange(n) % 2 == 0, lengths, np.maximum(lengths - 3, 0)).astype(np.int32)
    e = _host(eng.detect(_dev(packed), offsets=_dev(off), row_len=_dev(cut), params=p, want_info=True))
    for got, what in ((a, "strided"), (b, "strided + row_len"), (c, "packed")):
        _check(got, E, what)
    _check(e, dr.detect_rows(rows, dr.SMALL, row_len=cut), "packed + row_len")
    # a length beyond the stride (or negative) is clamped to the row
    wild = np.where(np.arange(n) % 2 == 0, stride + 5, -4).astype(np.int32)
    f = _host(eng.detect(_dev(rows), row_len=_dev(wild), params=p, want_info=True))
    _check(f, dr.detect_rows(rows, dr.SMALL, row_len=np.where(wild < 0, 0, stride)), "clamped row_len")
    del torch


@functools.lru_cache(maxsize=None)
def _adc_reads(n=64):
    """int16 reads whose calibrated rows look like the synthetic traces, per-read offset / scale; one read calibrates to NaN"""
    rows = _synth()[0][:n]
    rng = np.random.default_rng(11)
    stride = rows.shape[1]
    scale = rng.uniform(0.15, 0.25, n).astype(np.float32)
    offset = rng.integers(-260, -200, n).astype(np.float32)
    row_len = (~np.isnan(rows)).sum(axis=1).astype(np.int32)
    adc = np.zeros((n, stride), dtype=np.int16)
    live = ~np.isnan(rows)
    est = np.rint(np.where(live, rows, 0) / scale[:, None] - offset[:, None])
    adc[live] = np.clip(est, -32768, 32767).astype(np.int16)[live]
    adc[~live] = 12345          # behind row_len: never read
    offset[5] = np.nan
    row_len[6], row_len[7] = 0, stride
    pa = sig_proc.calibrate_adc(adc, np.minimum(row_len, stride), offset, scale)
    return adc, row_len, offset, scale, pa, dr.detect_rows(pa, dr.DEFAULT)


def test_adc_twins_equal_the_float_rows():
    from warpdemux_amd import engine

    adc, row_len, offset, scale, pa, E = _adc_reads()
    eng, p = _eng(), _params(dr.DEFAULT)
    n, stride = adc.shape
    assert (E.code == dr.OK).sum() > 50 and E.code[5] == dr.SHORT and E.info[5, 0] == 0 and E.info[6, 0] == 0
    _check(_host(eng.detect(_dev(pa), params=p, want_info=True)), E, "float rows")
    shard = engine.AdcShard(adc=_dev(adc), row_len=_dev(row_len), offset=_dev(offset), scale=_dev(scale))
    _check(_host(eng.detect(shard, params=p, want_info=True)), E, "strided shard")
    odd = np.full((n, stride + 1), 777, dtype=np.int16)         # an odd stride: every other row starts off the 4-byte boundary
    odd[:, :stride] = adc
    shard = engine.AdcShard(adc=_dev(odd), row_len=_dev(row_len), offset=_dev(offset), scale=_dev(scale))
    _check(_host(eng.detect(shard, params=p, want_info=True)), E, "strided shard, odd stride")
    slot = (np.minimum(row_len, stride).astype(np.int64) + 7) // 8 * 8 + 8 * (np.arange(n) % 3)     # slices in multiples of 8, some roomy
    off = np.concatenate(([0], np.cumsum(slot)))
    packed = np.full(int(off[-1]), 23456, dtype=np.int16)
    for r in range(n):
        m = min(int(row_len[r]), stride)
        packed[off[r]:off[r] + m] = adc[r, :m]
    shard = engine.AdcShard(adc=_dev(packed), row_len=_dev(row_len), offset=_dev(offset), scale=_dev(scale), offsets=_dev(off))
    _check(_host(eng.detect(shard, params=p, want_info=True)), E, "packed shard")


def test_host_forms_equal_the_device_form():
    rows, lengths, E = _small()
    p = _params(dr.SMALL)
    o = sig_proc.detect_batch_arrays(rows, p)
    _check({f: getattr(o, f) for f in FIELDS}, E, "wdx_detect_batch")
    junk = np.where(np.isnan(rows), np.float32(-3.0), rows)
    o = sig_proc.detect_batch_arrays(junk, p, row_len=lengths)
    _check({f: getattr(o, f) for f in FIELDS}, E, "wdx_detect_batch with row_len")
    res = sig_proc.detect_batch(rows[:65], p)
    assert [r.success for r in res] == (E.ok[:65] == 1).tolist()
    assert [r.adapter_start for r in res] == [int(v) if v >= 0 else None for v in E.a_start[:65]]
    assert [r.adapter_end for r in res] == [int(v) if v >= 0 else None for v in E.a_end[:65]]
    assert [r.fail_reason for r in res] == [sig_proc.DETECT_FAIL_REASONS[int(c)] for c in E.code[:65]]
    adc, row_len, offset, scale, pa, Ea = _adc_reads()
    o = sig_proc.detect_batch_adc(adc, np.minimum(row_len, adc.shape[1]), offset, scale)
    _check({f: getattr(o, f) for f in FIELDS}, Ea, "wdx_detect_batch_adc")
    # only `code` is required
    code = np.full(3, -9, np.int32)
    pc = p.to_c()
    sig = np.ascontiguousarray(rows[:3])
    _lib.check(_lib.load().wdx_detect_batch(_lib.default_context().handle, _lib.ptr(sig), 3, sig.shape[1], None, C.byref(pc), None, None,
                                            None, _lib.ptr(code), None, None))
    assert np.array_equal(code, E.code[:3])


# ---- exact buffers --------------------------------------------------------------------------------------------------------------

def _frames(n, given, offset_elems=0):
    return {name: fr.framed((n, cols) if cols > 1 else (n,), dt, offset=offset_elems * np.dtype(dt).itemsize)
            for name, dt, cols in OUT_SPEC if name in given}


def _raw_rows(eng, sig_ptr, off_ptr, len_ptr, stride, n, pc, frames, stream=None):
    ptrs = [frames[name].ptr if name in frames else None for name, _, _ in OUT_SPEC]
    return eng.L.wdx_detect_rows(eng.ctx.handle, sig_ptr, off_ptr, len_ptr, stride, n, C.byref(pc) if pc is not None else None, *ptrs,
                                 stream if stream is not None else eng._stream())


@pytest.mark.parametrize("case", ["all", "code-only", "off-alignment", "packed", "adc"])
def test_outputs_stay_inside_exact_buffers(case):
    rows, lengths, E = _small()
    eng, pc, n = _eng(), _params(dr.SMALL).to_c(), 65
    given = ("code",) if case == "code-only" else FIELDS
    frames = _frames(n, given, 1 if case == "off-alignment" else 0)
    if case == "packed":
        off = np.concatenate(([0], np.cumsum(lengths[:n].astype(np.int64))))
        ins = dict(sig=fr.framed_input(np.concatenate([rows[r, :lengths[r]] for r in range(n)])), off=fr.framed_input(off))
        _lib.check(_raw_rows(eng, ins["sig"].ptr, ins["off"].ptr, None, 0, n, pc, frames))
    elif case == "adc":
        adc = np.where(np.isnan(rows[:n]), 0, rows[:n]).astype(np.int16)        # integer-valued pA: scale 1, offset 0
        ins = dict(adc=fr.framed_input(adc), row_len=fr.framed_input(lengths[:n]), offset=fr.framed_input(np.zeros(n, np.float32)),
                   scale=fr.framed_input(np.ones(n, np.float32)))
        desc = _lib.AdcDevInC(adc=ins["adc"].ptr, row_off=None, stride=adc.shape[1], row_len=ins["row_len"].ptr, offset=ins["offset"].ptr,
                              scale=ins["scale"].ptr, row_win=None)
        ptrs = [frames[name].ptr if name in frames else None for name, _, _ in OUT_SPEC]
        _lib.check(eng.L.wdx_detect_rows_adc(eng.ctx.handle, C.byref(desc), n, C.byref(pc), *ptrs, eng._stream()))
    else:
        ins = dict(sig=fr.framed_input(rows[:n]))
        _lib.check(_raw_rows(eng, ins["sig"].ptr, None, None, rows.shape[1], n, pc, frames))
    _torch().cuda.synchronize()
    damage = {k: f.damage() for k, f in {**frames, **ins}.items() if f.damage()}
    assert not damage, damage
    want = E.take(slice(0, n))
    for name in given:
        got, w = frames[name].numpy(), getattr(want, name)
        if name == "gain":
            got, w = got.view(np.int64), w.view(np.int64)
        assert np.array_equal(got, w), (case, name)


def test_no_reads_and_bad_parameters_write_nothing():
    rows, lengths, E = _small()
    eng, n = _eng(), 8
    sig = fr.framed_input(rows[:n])
    frames = _frames(n, FIELDS)
    good = dr.SMALL
    assert _raw_rows(eng, sig.ptr, None, None, rows.shape[1], 0, _params(good).to_c(), frames) == 0
    assert _raw_rows(eng, None, None, None, 0, 0, _params(good).to_c(), {}) == 0
    bad = [dict(max_obs_trace=0), dict(max_obs_trace=16385), dict(quant_per_pa=0.0), dict(quant_per_pa=float("nan")), dict(find_start=2),
           dict(step_win=0), dict(step_win=9), dict(polya_win=1025, min_obs_adapter=2000), dict(min_obs_adapter=1), dict(max_obs_adapter=7),
           dict(start_win=0), dict(start_win=257), dict(refine=-1), dict(refine=4097), dict(max_start=-1), dict(open_pore_pa=float("inf")),
           dict(min_shift_pa=float("-inf")), dict(max_polya_var=float("nan"))]
    for change in bad:
        pc = _lib.DetectParamsC(*[dict(good, **change)[f[0]] for f in _lib.DetectParamsC._fields_])
        assert _raw_rows(eng, sig.ptr, None, None, rows.shape[1], n, pc, frames) == _lib.WDX_ERR_INVALID, change
        host = {f: np.full(n * (4 if f == "info" else 1), 0x5A, dtype=dict((a, b) for a, b, _ in OUT_SPEC)[f]) for f in FIELDS}
        src = np.ascontiguousarray(rows[:n])
        rc = eng.L.wdx_detect_batch(eng.ctx.handle, _lib.ptr(src), n, src.shape[1], None, C.byref(pc), *[_lib.ptr(host[f]) for f in FIELDS])
        assert rc == _lib.WDX_ERR_INVALID and all((host[f] == host[f].dtype.type(0x5A)).all() for f in FIELDS), change
    assert _raw_rows(eng, sig.ptr, None, None, rows.shape[1], n, None, frames) == _lib.WDX_ERR_INVALID              # no parameters
    assert _raw_rows(eng, sig.ptr, None, None, rows.shape[1], n, _params(good).to_c(), {k: v for k, v in frames.items() if k != "code"}) \
        == _lib.WDX_ERR_INVALID                                                                                          # no code
    assert _raw_rows(eng, None, None, None, rows.shape[1], n, _params(good).to_c(), frames) == _lib.WDX_ERR_INVALID    # no rows
    _torch().cuda.synchronize()
    for name, f in frames.items():
        assert f.intact() and (f.payload == fr.OUT_FILL).all(), name
    with pytest.raises(ValueError):
        eng.detect(_dev(rows[:n]), params=sig_proc.DetectParams(refine=5000))


# ---- the stream contract ----------------------------------------------------------------------------------------------------------

def test_stream_contract():
    """Behind a delay on the caller's stream the call returns at once and reads its rows in stream order (they arrive behind the
    delay); a delay pending on another stream is neither waited for nor disturbed."""
    torch = _torch()
    rows, lengths, E = _small()
    eng, p, n = _eng(), _params(dr.SMALL), 65
    real, decoy = _dev(rows[:n]), _dev(rows[n:2 * n])
    sig = torch.empty_like(real)
    _host(eng.detect(real, params=p, want_info=True))       # (warm: the code object is loaded)
    A, B, log = so.side_streams()
    print("\n".join(log))
    ev = so.late(A, [sig], [real], [decoy], 100.0)
    with torch.cuda.stream(A):
        d = eng.detect(sig, params=p, want_info=True)
    assert not ev.query(), "the call returned only after the delay on its stream had run"
    A.synchronize()
    _check({f: getattr(d, f).cpu().numpy() for f in FIELDS}, E.take(slice(0, n)), "behind the delay")
    # another stream's pending work
    so.delay(B, 200.0)
    with torch.cuda.stream(B):
        evB = torch.cuda.Event()
        evB.record(B)
    with torch.cuda.stream(A):
        d = eng.detect(real, params=p, want_info=True)
    A.synchronize()
    assert not evB.query(), "the call waited for another stream"
    _check({f: getattr(d, f).cpu().numpy() for f in FIELDS}, E.take(slice(0, n)), "beside a busy stream")
    B.synchronize()


# ---- composition ------------------------------------------------------------------------------------------------------------------

def test_detect_then_demux_without_crossing_the_bus():
    torch = _torch()
    rows, E = _synth()
    eng = _eng()
    sig = _dev(rows)
    d = eng.detect(sig)
    assert d.info is None and d.gain is None
    kw = dict(stride=rows.shape[1], max_len=8192, want_fpt=True)
    got = eng.demux(sig, d.a_start, d.a_end, ok=d.ok, **kw)
    want = eng.demux(sig, _dev(E.a_start), _dev(E.a_end), ok=_dev(E.ok), **kw)
    torch.cuda.synchronize()
    print("fingerprinted reads: %d of %d" % (int((want.status == 0).sum()), rows.shape[0]))
    assert int((want.status == 0).sum()) > 0 and int((want.status != 0).sum()) > 0
    for f in ("status", "call"):
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    assert torch.equal(got.dist.view(torch.int32), want.dist.view(torch.int32))
    assert torch.equal(got.fpt.view(torch.int64), want.fpt.view(torch.int64))
    assert torch.equal(d.a_start.cpu(), torch.from_numpy(E.a_start)) and torch.equal(d.a_end.cpu(), torch.from_numpy(E.a_end))
