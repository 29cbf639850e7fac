"""The int16 ADC way in, as far as it goes without a GPU: the new symbols, the NumPy statement of the calibration
contract (`sig_proc.calibrate_adc`), the int16 ring geometry of the feeder, and every argument check of the new entry
points -- which are host arithmetic and must answer WDX_ERR_INVALID before (and without) a device."""
import ctypes as C
import mmap
from fractions import Fraction

import numpy as np
import pytest

from warpdemux_amd import _lib, sig_proc

NEW = ["wdx_demux_submit_adc", "wdx_fingerprint_batch_adc", "wdx_demux_batch_adc", "wdx_calibrate_adc_dev", "wdx_feeder_run_adc"]


def test_new_symbols_are_exported_and_bound():
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS
        f = getattr(L, name)
        assert f.argtypes is not None and f.restype is C.c_int, name
    assert L.wdx_abi_version() == _lib.ABI_VERSION == 4
    assert C.sizeof(_lib.FeederGeometryC) == 40          # the format field took the place of the padding word


def _formula(adc, row_len, offset, scale, stride):
    """the contract, element by element on NumPy float32 scalars: float32 add, then float32 multiply"""
    out = np.full((adc.shape[0], stride), np.nan, dtype=np.float32)
    for r in range(adc.shape[0]):
        for i in range(int(row_len[r])):
            s = np.float32(np.float32(adc[r, i]) + np.float32(offset[r]))
            out[r, i] = np.float32(np.float32(scale[r]) * s)
    return out


def _round_f32(x: Fraction) -> np.float32:
    """x rounded ONCE to float32 (nearest, ties to even), in exact rational arithmetic"""
    c = np.float32(float(x))
    best = None
    for cand in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        err = abs(Fraction(float(cand)) - x)
        even = (int(np.float32(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, np.float32(cand))
    return best[1]


def test_calibrate_adc_is_the_two_rounding_formula():
    rng = np.random.default_rng(1)
    n, width, stride = 6, 40, 48
    adc = rng.integers(-32768, 32768, size=(n, width)).astype(np.int16)
    adc[0, :4] = [-32768, 32767, 0, -1]                       # the int16 extremes
    row_len = np.array([40, 0, 17, 40, 1, 33], dtype=np.int32)
    offset = np.array([-243.0, 12.3, -0.5, 7.77, 1e-3, -32768.25], dtype=np.float32)   # integer and non-integer offsets
    scale = np.array([0.1755, 0.17551, 0.2, 1.0, 3.0517578e-05, 0.1462], dtype=np.float32)
    got = sig_proc.calibrate_adc(adc, row_len, offset, scale, stride=stride)
    want = _formula(adc, row_len, offset, scale, stride)
    assert got.dtype == np.float32 and got.shape == (n, stride)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))           # NaNs included: the same quiet NaN
    for r in range(n):
        assert np.isfinite(got[r, :row_len[r]]).all() and np.isnan(got[r, row_len[r]:]).all()
    assert np.array_equal(sig_proc.calibrate_adc(adc, row_len, offset, scale)[:, :width].view(np.uint32),
                          want[:, :width].view(np.uint32))
    # a control: a sample on which ONE rounding (what a fused multiply-add of the whole expression would give) differs
    # from the contract's two -- found by search, so that the case is known to be one
    off, sc = np.float32(12.3), np.float32(0.1755)
    found = None
    for x in range(-32768, 32768):
        two = np.float32(sc * np.float32(np.float32(x) + off))
        one = _round_f32(Fraction(float(sc)) * (Fraction(x) + Fraction(float(off))))
        if two.view(np.uint32) != one.view(np.uint32):
            found = (x, two, one)
            break
    assert found is not None, "no sample separates one rounding from two"
    x, two, one = found
    assert two != one
    ctl = sig_proc.calibrate_adc(np.array([[x]], dtype=np.int16), [1], [off], [sc])
    assert ctl[0, 0].view(np.uint32) == two.view(np.uint32) and ctl[0, 0].view(np.uint32) != one.view(np.uint32)
    # what the helper refuses
    with pytest.raises(ValueError):
        sig_proc.calibrate_adc(adc.astype(np.int32), row_len, offset, scale)
    with pytest.raises(ValueError):
        sig_proc.calibrate_adc(adc, row_len[:-1], offset, scale)
    with pytest.raises(ValueError):
        sig_proc.calibrate_adc(adc, np.full(n, width + 1), offset, scale)
    with pytest.raises(ValueError):
        sig_proc.calibrate_adc(adc, row_len, offset, scale, stride=width - 1)


def _ring(fmt, n_slots=2, max_reads=10, max_stride=100, n_refs=4):
    L = _lib.load()
    geo = _lib.FeederGeometryC(n_slots, 0, 0, fmt, max_reads, max_stride, n_refs)
    n = L.wdx_feeder_ring_bytes(C.byref(geo))
    assert n > 0 and n % 4096 == 0
    m = mmap.mmap(-1, n)
    base = C.c_void_p(C.addressof(C.c_char.from_buffer(m)))
    pc = sig_proc.SegParams().to_c()
    _lib.check(L.wdx_feeder_ring_init(base, n, C.byref(geo), C.byref(pc)))
    return L, m, base


def test_int16_ring_is_smaller_and_still_holds_its_samples():
    L = _lib.load()
    for n_slots, max_reads, max_stride in ((2, 10, 100), (16, 1000, 10000), (3, 7, 4097)):
        f32 = _lib.FeederGeometryC(n_slots, 25, 11, _lib.FEEDER_SAMPLES_FLOAT32, max_reads, max_stride, 10)
        i16 = _lib.FeederGeometryC(n_slots, 25, 11, _lib.FEEDER_SAMPLES_INT16, max_reads, max_stride, 10)
        a, b = L.wdx_feeder_ring_bytes(C.byref(f32)), L.wdx_feeder_ring_bytes(C.byref(i16))
        assert 0 < b < a and b >= n_slots * max_reads * max_stride * 2, (a, b)
    bad = _lib.FeederGeometryC(2, 0, 0, 2, 10, 100, 4)          # an unknown sample format
    assert L.wdx_feeder_ring_bytes(C.byref(bad)) == 0


def _desc(n=3, stride=64, **over):
    a = dict(adc=np.zeros((n, stride), np.int16), row_len=np.full(n, stride, np.int32), offset=np.zeros(n, np.float32),
             scale=np.ones(n, np.float32), row_off=None, row_win=None, a_s=np.zeros(n, np.int32), a_e=np.full(n, 50, np.int32), ok=None)
    a.update(over)
    d = _lib.MinibatchAdcInC(_lib.addr(a["adc"]), n, stride, _lib.addr(a["row_len"]), _lib.addr(a["offset"]), _lib.addr(a["scale"]),
                             _lib.addr(a["row_off"]), _lib.addr(a["row_win"]), _lib.addr(a["a_s"]), _lib.addr(a["a_e"]), _lib.addr(a["ok"]))
    return d, a


BAD_DESCRIPTORS = [
    (dict(row_len=None), "row_len"),
    (dict(offset=None), "offset and scale"),
    (dict(scale=None), "offset and scale"),
    (dict(row_len=np.array([64, 65, 64], np.int32)), r"row_len\[1\] = 65"),
    (dict(row_len=np.array([64, -1, 64], np.int32)), r"row_len\[1\] = -1"),
    (dict(row_off=np.array([0, 64, 132, 192], np.int64)), "multiples of 8"),
    (dict(row_off=np.array([0, 64, 56, 192], np.int64)), "multiples of 8"),
    (dict(row_off=np.array([0, 64, 120, 192], np.int64)), "does not fit"),        # row 1 has 56 samples for row_len 64
    (dict(row_win=np.full(3, 64, np.int32)), "row_win"),
]


@pytest.mark.parametrize("over,msg", BAD_DESCRIPTORS)
def test_descriptor_checks_answer_invalid_without_a_device(over, msg):
    """no context is passed: a descriptor that is refused never reaches the context check, let alone a device"""
    L = _lib.load()
    pc = sig_proc.SegParams().to_c()
    d, keep = _desc(**over)
    st = np.zeros(3, np.int32)
    f = np.zeros((3, 25))
    calls = (lambda: L.wdx_demux_submit_adc(None, 0, C.byref(d), C.byref(pc), 4, 0),
             lambda: L.wdx_fingerprint_batch_adc(None, C.byref(d), C.byref(pc), _lib.ptr(f), _lib.ptr(f), _lib.ptr(f), _lib.ptr(st)),
             lambda: L.wdx_demux_batch_adc(None, C.byref(d), C.byref(pc), 4, None, None, _lib.ptr(st), _lib.ptr(st)))
    for call in calls:
        assert call() == _lib.WDX_ERR_INVALID
        with pytest.raises(ValueError, match=msg):
            _lib.check(_lib.WDX_ERR_INVALID)
    del keep


def test_a_good_descriptor_gets_as_far_as_the_context_check():
    L = _lib.load()
    pc = sig_proc.SegParams().to_c()
    d, keep = _desc()
    assert L.wdx_demux_submit_adc(None, 0, C.byref(d), C.byref(pc), 4, 0) == _lib.WDX_ERR_INVALID
    assert L.wdx_last_error() == b"null context"
    assert L.wdx_demux_submit_adc(None, 0, None, C.byref(pc), 4, 0) == _lib.WDX_ERR_INVALID
    assert b"null minibatch" in L.wdx_last_error()
    one = np.zeros(8, np.float32)
    for args, msg in (((None, None, None, 64, 3, one.ctypes.data, one.ctypes.data, one.ctypes.data, None), b"bad arguments"),
                      ((one.ctypes.data, None, None, 64, 3, one.ctypes.data, one.ctypes.data, one.ctypes.data, None), b"row_len"),
                      ((one.ctypes.data, None, one.ctypes.data, 64, 3, None, one.ctypes.data, one.ctypes.data, None), b"offset and scale"),
                      ((one.ctypes.data, None, one.ctypes.data, 64, 3, one.ctypes.data, None, one.ctypes.data, None), b"offset and scale"),
                      ((one.ctypes.data, None, one.ctypes.data, 64, 3, one.ctypes.data, one.ctypes.data, one.ctypes.data, None), b"null context")):
        assert L.wdx_calibrate_adc_dev(None, *args) == _lib.WDX_ERR_INVALID
        assert msg in L.wdx_last_error(), (msg, L.wdx_last_error())
    del keep


def _jobs(n=3, stride=50):
    st = np.zeros(n, np.int32)
    a = np.zeros(n, np.int32)
    sig = np.zeros((n, stride), np.float32)
    adc = np.zeros((n, stride), np.int16)
    rl = np.full(n, stride, np.int32)
    cal = np.ones(n, np.float32)
    fjob = _lib.FeederJobC(sig.ctypes.data, n, stride, a.ctypes.data, a.ctypes.data, None, 0, 0, st.ctypes.data, st.ctypes.data,
                           None, None, None, None, None, None, None)

    def ajob(row_len=rl, offset=cal, scale=cal):
        return _lib.FeederJobAdcC(adc.ctypes.data, n, stride, _lib.addr(row_len), _lib.addr(offset), _lib.addr(scale), a.ctypes.data,
                                  a.ctypes.data, None, 0, 0, st.ctypes.data, st.ctypes.data, None, None, None, None, None, None, None)
    return fjob, ajob, (st, a, sig, adc, rl, cal)


def test_job_and_ring_formats_must_match():
    fjob, ajob, keep = _jobs()
    L, m16, ring16 = _ring(_lib.FEEDER_SAMPLES_INT16)
    with pytest.raises(ValueError, match="float32 rows on a ring laid out for int16"):
        _lib.check(L.wdx_feeder_run(ring16, C.byref(fjob)))
    sig, a, d, c = keep[2], keep[1], np.zeros((3, 4), np.float32), np.zeros(3, np.int32)
    with pytest.raises(ValueError, match="float32 rows on a ring laid out for int16"):
        _lib.check(L.wdx_feeder_demux(ring16, sig.ctypes.data, 3, 50, a.ctypes.data, a.ctypes.data, None, 4, d.ctypes.data,
                                      c.ctypes.data, c.ctypes.data))
    L, m32, ring32 = _ring(_lib.FEEDER_SAMPLES_FLOAT32)
    job = ajob()
    with pytest.raises(ValueError, match="int16 rows on a ring laid out for float32"):
        _lib.check(L.wdx_feeder_run_adc(ring32, C.byref(job)))
    del ring16, ring32


def test_feeder_run_adc_checks_its_job_without_a_feeder():
    fjob, ajob, keep = _jobs()
    L, m, ring = _ring(_lib.FEEDER_SAMPLES_INT16)
    for kw, msg in ((dict(row_len=None), "row_len"), (dict(offset=None), "offset and scale"), (dict(scale=None), "offset and scale"),
                    (dict(row_len=np.array([50, 51, 50], np.int32)), r"row_len\[1\] = 51"),
                    (dict(row_len=np.array([-3, 50, 50], np.int32)), r"row_len\[0\] = -3")):
        job = ajob(**kw)
        with pytest.raises(ValueError, match=msg):
            _lib.check(L.wdx_feeder_run_adc(ring, C.byref(job)))
    with pytest.raises(ValueError, match="null job"):
        _lib.check(L.wdx_feeder_run_adc(ring, None))
    big = _lib.FeederJobAdcC(keep[3].ctypes.data, 11, 50, keep[4].ctypes.data, keep[5].ctypes.data, keep[5].ctypes.data,
                             keep[1].ctypes.data, keep[1].ctypes.data, None, 0, 0, keep[0].ctypes.data, keep[0].ctypes.data,
                             None, None, None, None, None, None, None)
    with pytest.raises(ValueError, match="row_len|do not fit"):
        _lib.check(L.wdx_feeder_run_adc(ring, C.byref(big)))
    # a good job on a ring nobody serves, after a stop: told, not hung (as for float32 rows)
    _lib.check(L.wdx_feeder_stop(ring))
    job = ajob()
    with pytest.raises(_lib.WdxNoDevice, match="feeder"):
        _lib.check(L.wdx_feeder_run_adc(ring, C.byref(job)))
    del ring


def test_python_front_doors_check_every_array_before_passing_it_by_address():
    n, stride = 4, 32
    adc = np.zeros((n, stride), np.int16)
    rl, cal, a = np.full(n, stride, np.int32), np.ones(n, np.float32), np.zeros(n, np.int32)
    desc, m, kept = sig_proc.adc_minibatch(adc, rl, cal, cal, a, a, np.ones(n, np.uint8))
    assert m == n and desc.stride == stride and desc.adc == adc.ctypes.data and kept[0] is adc      # passed in place
    for bad in (dict(adc=adc.astype(np.float32)), dict(adc=adc[:, ::2]), dict(adc=adc[0]), dict(row_len=rl[:-1]),
                dict(offset=cal[:-1]), dict(scale=np.ones((n, 1), np.float32)), dict(adapter_start=a[:-1]),
                dict(adapter_end=np.zeros(n + 1, np.int32)), dict(success=np.ones(n - 1, np.uint8)),
                dict(success=np.ones((n, 2), np.uint8)), dict(row_win=rl)):
        kw = dict(adc=adc, row_len=rl, offset=cal, scale=cal, adapter_start=a, adapter_end=a, success=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            sig_proc.adc_minibatch(**kw)
    flat = np.zeros(n * stride, np.int16)
    off = np.arange(n + 1, dtype=np.int64) * stride
    desc, m, kept = sig_proc.adc_minibatch(flat, rl, cal, cal, a, a, None, row_off=off, row_win=rl)
    assert m == n and desc.row_off == kept[4].ctypes.data and desc.row_win == kept[5].ctypes.data
    for bad in (dict(row_off=off[:-1]), dict(row_off=off * 2), dict(adc=adc, row_off=off), dict(row_off=off, row_win=rl[:-1])):
        kw = dict(adc=flat, row_len=rl, offset=cal, scale=cal, adapter_start=a, adapter_end=a, success=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            sig_proc.adc_minibatch(**kw)


def test_float_front_doors_check_every_array_before_passing_it_by_address():
    """the float32 counterpart: the shared check and the three blocking calls over it.  Every refusal is a ValueError raised
    before a context is asked for -- on a machine without a device a WdxError here would mean the check came too late"""
    from warpdemux_amd import _marshal

    n, stride = 4, 32
    sig, a, ok = np.zeros((n, stride), np.float32), np.zeros(n, np.int32), np.ones(n, np.uint8)
    got = _marshal.minibatch(sig, a, a, ok)
    assert got[4:] == (n, stride) and got[0] is sig and got[1].dtype == got[2].dtype == np.int32 and got[3].dtype == np.uint8
    assert _marshal.minibatch(sig.astype(np.float64)[:, ::2], list(a), a, None)[3:] == (None, n, stride // 2)
    params = sig_proc.SegParams()
    refine = sig_proc.RefineParams(query=np.linspace(-1.0, 1.0, 84))
    doors = (_marshal.minibatch,
             lambda s, a_s, a_e, su: sig_proc.fingerprint_batch(s, a_s, a_e, params, success=su),
             lambda s, a_s, a_e, su: sig_proc.fingerprint_refine_batch(s, a_s, a_e, params, refine, success=su),
             lambda s, a_s, a_e, su: sig_proc.demux_batch(s, a_s, a_e, params, success=su))
    for door in doors:
        for bad in (dict(signals=sig[0]), dict(adapter_start=a[:-1]), dict(adapter_end=np.zeros(n + 1, np.int32)),
                    dict(success=np.ones(n - 1, np.uint8)), dict(success=np.ones((n, 2), np.uint8))):
            kw = dict(signals=sig, adapter_start=a, adapter_end=a, success=ok)
            kw.update(bad)
            with pytest.raises(ValueError):
                door(kw["signals"], kw["adapter_start"], kw["adapter_end"], kw["success"])
