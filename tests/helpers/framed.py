"""Exact device buffers between guard bands (tests/test_gpu_buffer_bounds.py).

`framed(nbytes_or_shape, dtype, fill)` is one uint8 device tensor laid out as [front guard | payload | back guard].  The
payload holds exactly the bytes asked for, so the back guard starts on the very next byte, aligned or not; each guard is
GUARD bytes (a multiple of 512: the payload keeps torch's base alignment) plus, with ``offset``, that many bytes in
front -- a payload whose address is ``offset`` modulo 512.  The guards hold a seeded, non-constant byte pattern, so a
kernel that happens to store one byte value everywhere cannot leave them intact; the payload is filled with a stated byte.

Behind an INPUT the back guard decodes as what a load past the last element must not profit from: NaN for float32 /
float64 (random mantissa bits under a quiet-NaN exponent), 32767 for int16.  A result that moves with what lies past an
input is then a mismatch with the reference, not luck.

`work_pieces(n, K)` restates, in Python, where wdx_demux_dev's layout puts the fingerprint stage's counters inside d_work
(warpdemux_amd/csrc/wdx_work_layout.h); tests/test_work_layout_host.py pins it against the header."""
import numpy as np

GUARD = 64 * 1024
assert GUARD % 512 == 0 and GUARD >= 64 * 1024
OUT_FILL = 0xA5     # no legal status, call or index, and not the library's NaN

_BYTES = {"float32": 4, "float64": 8, "int16": 2, "int32": 4, "int64": 8, "uint8": 1}
_patterns = {}


def _pattern(kind, length, phase=0):
    """`length` guard bytes of `kind` on the host: "random", or element-wise NaN / 32767 behind inputs (the pattern
    starts on an element boundary: a payload of whole elements ends on one)"""
    key = (kind, length, phase)
    if key not in _patterns:
        rng = np.random.default_rng(0x5EED + 17 * phase)
        raw = rng.integers(0, 256, length + 8, dtype=np.uint8)
        if kind == "nan32":
            raw[2::4], raw[3::4] = 0xC0 | (raw[2::4] & 0x3F), 0x7F
        elif kind == "nan64":
            raw[6::8], raw[7::8] = 0xF8 | (raw[6::8] & 0x07), 0x7F
        elif kind == "i16max":
            raw[0::2], raw[1::2] = 0xFF, 0x7F
        else:
            assert kind == "random", kind
        _patterns[key] = raw[:length].copy()
    return _patterns[key]


def guard_kind(dtype):
    """the back guard of an INPUT of this dtype"""
    return {"float32": "nan32", "float64": "nan64", "int16": "i16max"}.get(str(np.dtype(dtype)), "random")


class Framed:
    def __init__(self, nbytes, dtype, fill, shape, back, offset):
        import torch

        self.torch = torch
        self.nbytes, self.dtype, self.shape, self.fill = int(nbytes), np.dtype(dtype), shape, fill
        self.front = GUARD + int(offset)
        self._front = torch.from_numpy(_pattern("random", self.front, 1)).cuda()
        self._back = torch.from_numpy(_pattern(back, GUARD)).cuda()
        self.buf = torch.empty(self.front + self.nbytes + GUARD, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 512 == 0
        self.buf[:self.front] = self._front
        self.buf[self.front + self.nbytes:] = self._back
        self.payload.fill_(fill)

    @property
    def payload(self):
        """the payload's bytes (a view)"""
        return self.buf[self.front:self.front + self.nbytes]

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.front

    def view(self, dtype=None, shape=None):
        """the payload as a typed view (its address must suit the dtype)"""
        dtype = np.dtype(dtype or self.dtype)
        shape = self.shape if shape is None else shape
        assert self.ptr % dtype.itemsize == 0 and self.nbytes % dtype.itemsize == 0
        t = self.payload.view(getattr(self.torch, str(dtype)))
        return t if shape is None else t.view(*shape)

    def numpy(self, dtype=None, shape=None):
        """a host copy of the payload, typed"""
        a = self.payload.cpu().numpy().view(np.dtype(dtype or self.dtype))
        shape = self.shape if shape is None else shape
        return a if shape is None else a.reshape(shape)

    def set(self, array):
        """the payload := these bytes (an input's values, a histogram's start)"""
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        assert raw.size == self.nbytes, (raw.size, self.nbytes)
        if raw.size:
            self.payload.copy_(self.torch.from_numpy(raw))
        return self

    def damage(self):
        """[] when both guards hold their pattern, else [(side, first damaged offset, last damaged offset)]: front offsets
        count back from the payload's first byte (1 = the byte just before it), back offsets on from its end (0 = the very
        next byte)"""
        self.torch.cuda.synchronize()
        out = []
        for side, got, want in (("front", self.buf[:self.front], self._front), ("back", self.buf[self.front + self.nbytes:], self._back)):
            bad = (got != want).nonzero().flatten()
            if bad.numel():
                lo, hi = int(bad[0]), int(bad[-1])
                out.append((side, self.front - hi, self.front - lo) if side == "front" else (side, lo, hi))
        return out

    def intact(self):
        return self.damage() == []


def framed(nbytes_or_shape, dtype="uint8", fill=OUT_FILL, back="random", offset=0):
    """[front guard | payload | back guard] on the device.  An int asks for that many BYTES, a shape for that many elements
    of `dtype`; ``fill`` the byte the payload starts with; ``back`` the back guard's kind (`guard_kind(dtype)` behind an
    input); ``offset`` moves the payload that many bytes off its 512-byte boundary."""
    dtype = np.dtype(dtype)
    if isinstance(nbytes_or_shape, (int, np.integer)):
        nbytes, shape = int(nbytes_or_shape), None
    else:
        shape = tuple(int(v) for v in nbytes_or_shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    return Framed(nbytes, dtype, fill, shape, back, offset)


def framed_input(array, offset=0):
    """an input's values in a frame that ends on its last element, NaN / 32767 behind it"""
    a = np.ascontiguousarray(array)
    return framed(a.shape, a.dtype, 0, guard_kind(a.dtype), offset).set(a)


# ---- the layout of d_work, restated (warpdemux_amd/csrc/wdx_work_layout.h) ------------------------------------------------------
ROW_MAJOR_MIN_READS, SPLIT_REC, SPLIT_SLICE, CLIP_REC, REFINE_REC, N_COUNTERS = 8192, 4624, 524288, 16, 1632, 8
COUNTER_NAMES = ("slow", "big0", "big1", "retry", "big2", "back", "back_tie", "back_list")


def _up(v, m):
    return (v + m - 1) // m * m


def work_pieces(n, K, with_T=None):
    """byte offsets inside d_work for a float32 call of n reads: fp_ws (the fingerprint workspace, whose first 32 bytes are
    the eight counters), the pieces inside it, plain / refine sizes and the hand-over records' offset"""
    with_T = (n < ROW_MAJOR_MIN_READS) if with_T is None else with_T
    ld = _up(max(n, 1), 64)
    fptT = _up(n * K * 8, 256)
    flags = fptT + (K * ld * 8 if with_T else 0)
    fp_ws = flags + (_up(ld, 256) if with_T else 0)
    m = max(n, 0)
    count, clip = 0, 4 * N_COUNTERS
    lists = [clip + CLIP_REC * m + 4 * m * i for i in range(6)]
    split = _up(lists[5] + 4 * m, 16)
    dbg = split + SPLIT_REC * min(m, SPLIT_SLICE)
    fp_bytes = dbg + 64
    plain = n * K * 8 + (K * ld * 8 + ld if with_T else 0) + 512 + fp_bytes
    return dict(fp_ws=fp_ws, count=count, clip=clip, lists=lists, split=split, dbg=dbg, fp_bytes=fp_bytes, plain_bytes=plain,
                refine_off=_up(plain, 256), refine_bytes=_up(plain, 256) + REFINE_REC * m)


def counters(work, n, K, with_T=None):
    """the eight counters the fingerprint stage left at the front of its piece of this d_work frame, by name"""
    at = work_pieces(n, K, with_T)["fp_ws"]
    raw = work.payload[at:at + 4 * N_COUNTERS].cpu().numpy().view(np.uint32)
    return dict(zip(COUNTER_NAMES, (int(v) for v in raw)))
