"""clip_bounds_kernel<64> / <80> / <96> (wdx_clip.hip) after the residency change -- the member list laid over the histogram,
the bin search reduced in stages of chunk rows, five / five / four waves per SIMD -- on the smallest windows at which the
aliasing and the restaged reduction can go wrong.  Every window is constructed so that the level of the select it is about
takes a known path:

  * the MEDIAN's first level bins the raw bit pattern; with every sample in [64, 128), the smallest exactly 64.0 and the
    largest the last float below 128, bin B is the 4096 patterns from 0x42800000 + 4096 B (shift 12, 2048 bins)
  * the MAD's first level bins |x - med| * (2047 / dmax) linearly; with med == 96 and dmax == 2047 / 64 the scale is 64
    exactly and bin B holds the deviations in [B / 64, (B + 1) / 64)

so the rank-k key is put into a chosen bin (first / last bin of each of the 16 chunk rows, bin 0, bin 2047, both halves of a
bin pair) with a chosen number of members (1, 63, 64 -- ranked directly --, 65 -- one more level --, hundreds of copies of
one value, two interleaved values).  The reference is NumPy's nanmedian / MAD and sig_proc.py:421-431's bounds, computed here;
lo, hi, cmax and flag of EVERY constructed read are compared bit for bit (a read the kernel must refuse is compared with the
refusal record), and the reference's bounds are checked to be finite before the GPU sees a read.
Needs a real MI355X: run with `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

from warpdemux_amd import _lib, sig_proc

pytestmark = pytest.mark.gpu

CAPS = [4096, 5120, 6144]                      # clip_bounds_kernel<64>, <80>, <96>
P0 = 0x42800000                                # 64.0f
PMAX = 0x42FFFFFF                              # the last float below 128
MED = np.float32(96.0)
GRID = 2.0 ** -17                              # ulp of [64, 128): deviations from 96 on this grid are exact
DMAX_IDX = 2047 * 2048                         # dmax = 2047 / 64 on the grid
BINS = sorted({0, 2047, 1000, 1001} | {128 * q for q in range(16)} | {128 * q + 127 for q in range(16)})
PARAMS = sig_proc.SegParams(padding=0, outlier_thresh=5.0, clip_bounds="float32")
REC = np.dtype([("lo", "<f4"), ("hi", "<f4"), ("cmax", "<f4"), ("flag", "<i4")])


def _run(rows, cap, params):
    """wdx_selftest_clip_dev over the packed windows (as tests/test_gpu_clip.py::_run) -> one record per window."""
    import torch

    lens = np.array([r.size for r in rows], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = len(rows)
    d_sig = torch.from_numpy(np.concatenate(rows).astype(np.float32)).cuda()
    d_off = torch.from_numpy(off).cuda()
    d_as = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ae = torch.from_numpy(lens.astype(np.int32)).cuda()
    d_rec = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
    ctx = _lib.default_context()
    pc = params.to_c()
    _lib.check(_lib.load().wdx_selftest_clip_dev(ctx.handle, C.c_void_p(d_sig.data_ptr()), C.c_void_p(d_off.data_ptr()), 0, n,
                                                 C.c_void_p(d_as.data_ptr()), C.c_void_p(d_ae.data_ptr()), C.byref(pc), cap,
                                                 C.c_void_p(d_rec.data_ptr()), None))
    torch.cuda.synchronize()
    return d_rec.cpu().numpy().view(REC).reshape(n)


def _rank(n):
    return n // 2 if n & 1 else n // 2 - 1


def _split(n, k, c, lo_fixed, hi_fixed, no_below, no_above):
    """Number of keys below the bin so that ranks L .. L + c - 1 are the bin's and hold rank k."""
    if no_below:
        L = 0
    elif no_above:
        L = n - c
    else:
        L = min(max(k - (c - 1) // 2, lo_fixed), n - c - hi_fixed)
    assert L >= (0 if no_below else lo_fixed) and n - L - c >= (0 if no_above else hi_fixed), (n, k, c, L)
    assert L <= k < L + c, (n, k, c, L)
    return L


def _median_window(rng, n, B, members):
    """n samples in [64, 128), min 64.0, max the last float below 128: the median's rank-k key lies in bin B of the first
    level, whose members are `members` (bit patterns)."""
    members = np.asarray(members, dtype=np.int64)
    assert ((members - P0) >> 12 == B).all()
    c, k = members.size, _rank(n)
    L = _split(n, k, c, 1, 1, B == 0, B == 2047)
    H = n - L - c
    parts = [members]
    if L:
        parts += [[P0], P0 + rng.integers(0, B * 4096, L - 1)]
    if H:
        parts += [[PMAX], P0 + rng.integers((B + 1) * 4096, 2048 * 4096, H - 1)]
    pat = np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])
    assert pat.size == n and pat.min() == P0 and pat.max() == PMAX
    x = rng.permutation(pat.astype(np.uint32)).view(np.float32)
    s = np.sort(x.view(np.uint32).astype(np.int64))
    assert (s[k] - P0) >> 12 == B and int(np.sum((s - P0) >> 12 == B)) == c
    return x


def _mad_window(rng, n, B, member_idx):
    """n samples 96 +/- d (d on the 2^-17 grid, the largest 2047 / 64), median exactly 96: the MAD's rank-k key lies in bin B
    of the first (linear) level, whose members are the deviations `member_idx` (grid indices; bin B is [2048 B, 2048 B + 2047])."""
    member_idx = np.asarray(member_idx, dtype=np.int64)
    assert (member_idx >> 11 == B).all() and member_idx.max() <= DMAX_IDX
    odd = n & 1
    base = np.array([0] if odd else [1, 1], dtype=np.int64)   # the middle sample(s): 96, or 96 -/+ 2^-17
    k = _rank(n)
    if B == 0:                                                # the middle keys are members of bin 0
        member_idx = np.concatenate([base, member_idx])
        base = base[:0]
    c = member_idx.size
    L = _split(n, k, c, base.size, 1, B == 0, B == 2047)
    H = n - L - c
    parts = [member_idx, base]
    if L - base.size:
        parts.append(rng.integers(1, B * 2048, L - base.size))
    if H:
        parts += [[DMAX_IDX], rng.integers((B + 1) * 2048, DMAX_IDX + 1, H - 1)]
    d = np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])
    assert d.size == n and d.max() == DMAX_IDX
    # signs: the middle pair one of each, the others split evenly (any assignment leaves the median at 96)
    mid = np.zeros(n, dtype=bool)
    first = int(np.flatnonzero(d == (0 if odd else 1))[0])
    if odd:
        mid[first] = True
        sign = np.zeros(n)
        rest = np.flatnonzero(~mid)
    else:
        second = int(np.flatnonzero(d == 1)[1])
        mid[[first, second]] = True
        sign = np.zeros(n)
        sign[first], sign[second] = -1, 1
        rest = np.flatnonzero(~mid)
    rest = rng.permutation(rest)
    sign[rest[: rest.size // 2]] = -1
    sign[rest[rest.size // 2:]] = 1
    x = (96.0 + sign * d * GRID).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), 96.0 + sign * d * GRID)          # representable
    x = rng.permutation(x)
    assert np.nanmedian(x) == MED
    key = np.abs(x - MED)
    assert key.max() == np.float32(2047 / 64) and np.float32(2047) / key.max() == np.float32(64)
    b = (key * np.float32(64)).astype(np.int64)
    assert np.sort(b)[k] == B and int(np.sum(b == B)) == c
    return x


def _members_pat(rng, B, kind):
    lo = P0 + B * 4096
    if kind == "copies":
        return np.full(300, lo + 1234)
    if kind == "two-values-gather":
        return np.tile([lo + 100, lo + 3000], 50)            # 100 in the bin -> a level -> 50 + 50, gathered
    if kind == "two-values-copies":
        return np.tile([lo + 100, lo + 3000], 150)           # 300 in the bin -> a level -> 150 copies -> sa == sb
    return lo + rng.choice(4096, int(kind), replace=False)


def _members_idx(rng, B, kind):
    lo = B * 2048
    if kind == "copies":
        return np.full(300, lo + 777)
    if kind == "two-values-gather":
        return np.tile([lo + 100, lo + 1900], 50)
    if kind == "two-values-copies":
        return np.tile([lo + 100, lo + 1900], 150)
    return lo + rng.choice(2048, int(kind), replace=False)


MEMBER_KINDS = ["1", "63", "64", "65", "copies", "two-values-gather", "two-values-copies"]


def _emulate_refusal(x):
    """The one-wave kernel's refusals (wdx_clip.hip): 2 = an infinity / NaN, 3 = negative samples it may not clamp to the
    smallest non-negative one (the median does not lie above it, or the MAD not below its key), else 0."""
    if not np.isfinite(x).all():
        return 2
    neg = np.signbit(x)
    if not neg.any():
        return 0
    if neg.all():
        return 2
    n, k = x.size, _rank(x.size)
    umn = x[~neg].min()
    cl = np.where(neg, umn, x).astype(np.float32)
    s = np.sort(cl)
    if s[k] == umn:
        return 3
    med = s[k] if n & 1 else np.float32((s[k] + s[k + 1]) / np.float32(2))
    keys = np.sort(np.abs(cl - med))
    if (keys[k] if n & 1 else keys[k + 1]) >= np.abs(umn - med):
        return 3
    return 0


def _expected(x, cap):
    """The record clip_bounds_kernel owes for window x: (lo, hi, cmax, flag)."""
    zero = np.float32(0)
    if not 256 <= x.size <= cap:
        return zero, zero, zero, 0
    refusal = _emulate_refusal(x)
    if refusal:
        return zero, zero, zero, refusal
    med = np.nanmedian(x)
    mad = np.nanmedian(np.abs(x - med))
    assert med.dtype == np.float32 and mad.dtype == np.float32
    tm = np.float32(PARAMS.outlier_thresh) * mad
    lo, hi = np.float32(med - tm), np.float32(med + tm)
    assert np.isfinite(lo) and np.isfinite(hi), "the reference's bounds are finite for every constructed read"
    cmin, cmax = np.clip(x.min(), lo, hi), np.clip(x.max(), lo, hi)
    gate = bool(lo <= hi and cmin > 0 and cmax < 3.0e38)
    if gate:
        fa = max(int(np.float32(cmin).view(np.uint32)) >> 23, 1)
        fb = int(np.float32(cmax).view(np.uint32)) >> 23
        gate = (fb - fa) + int(x.size).bit_length() <= 28
    return lo, hi, np.float32(cmax), 1 if gate else 3


@functools.lru_cache(maxsize=None)
def _windows():
    """[(family, tag, window, flag the case is built for or None)], built once."""
    rng = np.random.default_rng(8192)
    out = []
    for n in (1025, 1024):                                   # five / four groups of 256, odd / even
        k = _rank(n)
        for kind in MEMBER_KINDS:
            out.append(("members-median", (kind, n), _median_window(rng, n, 777, _members_pat(rng, 777, kind)), 1))
            out.append(("members-mad", (kind, n), _mad_window(rng, n, 777, _members_idx(rng, 777, kind)), 1))
        for B in BINS:
            # bin 0 / bin 2047 hold rank k only with every rank below / above it: more than half the window
            c = k + 5 if B == 0 else (n - k + 3 if B == 2047 else 5)
            pat = PMAX - np.arange(c) if B == 2047 else P0 + B * 4096 + np.sort(rng.choice(4095, c, replace=False)) + (B != 0)
            if B == 0:
                pat[0] = P0
            out.append(("bins-median", (B, n), _median_window(rng, n, B, pat), 1))
            idx = np.full(c, DMAX_IDX) if B == 2047 else B * 2048 + 1 + rng.choice(2047, c, replace=False)
            out.append(("bins-mad", (B, n), _mad_window(rng, n, B, idx), 1))
    for n in (256, 257, 511, 512, 513, 4095, 4096, 4097, 5119, 5120, 6143, 6144):
        for rep in range(2):
            x = (rng.normal(90, 12, n) + rng.normal(0, 2, n)).astype(np.float32)
            assert x.min() > 0
            out.append(("edges", (n, rep), x, None))
    for n in (1000, 1001):
        x = rng.normal(90, 3, n).astype(np.float32)
        x[17] = -25.0
        out.append(("negative", ("spike, median above", n), x, 1))
        x = np.concatenate([np.full(600, 70.0), rng.uniform(71, 110, n - 601), [-25.0]]).astype(np.float32)
        out.append(("negative", ("median at the clamped value", n), rng.permutation(x), 3))
        m = _rank(n) + 1     # rank k is the largest of the low cluster: all but k keys are at or above the clamped one's
        x = np.concatenate([rng.uniform(89, 90, m), rng.uniform(120, 290, n - m - 1), [-3.0]]).astype(np.float32)
        out.append(("negative", ("MAD not below the clamped key", n), rng.permutation(x), 3))
        for bad in (np.inf, -np.inf):
            x = rng.normal(90, 3, n).astype(np.float32)
            x[n // 3] = bad
            out.append(("negative", ("infinity", n), x, 2))
    return out


@functools.lru_cache(maxsize=None)
def _expected_all(cap):
    exp = []
    for fam, tag, x, want in _windows():
        e = _expected(x, cap)
        if want is not None:                                  # the case is what it claims to be
            assert e[3] == want, (fam, tag, e)
        exp.append(e)
    return exp


@functools.lru_cache(maxsize=None)
def _records(cap):
    exp = _expected_all(cap)                                  # (the CPU-side checks come before the GPU sees a read)
    return _run([w[2] for w in _windows()], cap, PARAMS), exp


def _compare(cap, family):
    rec, exp = _records(cap)
    compared = 0
    for (fam, tag, x, _), r, (lo, hi, cmax, flag) in zip(_windows(), rec, exp):
        if fam != family:
            continue
        got = (r["lo"].view(np.uint32), r["hi"].view(np.uint32), r["cmax"].view(np.uint32), int(r["flag"]))
        want = (lo.view(np.uint32), hi.view(np.uint32), cmax.view(np.uint32), flag)
        assert got == want, (cap, fam, tag, x.size, r, lo, hi, cmax, flag)
        compared += 1
    assert compared == sum(1 for w in _windows() if w[0] == family) > 0   # no read left out
    return compared


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("level", ["median", "mad"])
def test_member_list_over_the_histogram(cap, level):
    """1, 63, 64, 65 members, copies of one value and two interleaved values in the bin of the median / of the MAD: the list
    is written over the dead histogram and read back whole; the next level (the MAD's after the median's) clears it."""
    assert _compare(cap, "members-" + level) == 2 * len(MEMBER_KINDS)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("level", ["median", "mad"])
def test_bin_search_in_stages_finds_every_chunk_row_edge(cap, level):
    """The rank-k key in the first and the last bin of each of the 16 chunk rows, bin 0, bin 2047 and both halves of a pair."""
    assert len(BINS) == 34
    assert _compare(cap, "bins-" + level) == 2 * len(BINS)


@pytest.mark.parametrize("cap", CAPS)
def test_group_edges_both_parities(cap):
    """Window lengths around the 256-sample groups and every capacity (a window longer than the capacity is left alone)."""
    _compare(cap, "edges")


@pytest.mark.parametrize("cap", CAPS)
def test_negative_sample_clamp_and_refusals(cap):
    """One negative spike below a median above it (answered), the median at the clamped value and the MAD at its key
    (CLIP_INEXACT), an infinity (CLIP_NAN_NEG): flag and the zeroed bounds compared as well."""
    _compare(cap, "negative")
