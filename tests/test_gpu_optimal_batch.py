"""The whole-read kernel of the optimal change-points (fingerprint_refine_optimal_kernel, WDX_OPT_REFINE_OPTIMAL_CPTS) at batch
size: workgroups that finish a second and a third read, every adapter-segmenting kernel in front of it, the parameter domain of
its own score tail, and the tile ends of that tail.  The reference is the helper's composition of the oracle's primitives
(tests/helpers/optimal_cpts.py:refine_batch) with the oracle's C statement of the rule evaluating the barcode tail
(wdx_oracle_optimal_cpts, pinned to the NumPy statement by tests/test_optimal_cpts_host.py).  Everything bit for bit, NaN by
position; no tolerances.

Reads as tests/test_gpu_refine.py:_reads makes them, with fixture g14's consensus: a random lead, the consensus or noise, a
random tail of levels, dwell times 2 d + 2 .. 4 d + 7, float32."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from helpers import optimal_cpts as oc, optimal_inputs as oi, optimal_plan as op
from warpdemux_amd import _lib, sig_proc

pytestmark = pytest.mark.gpu

NAMES = ("status", "fpt", "dwell", "stats", "refine_idx")
same = oi.same


@functools.lru_cache(maxsize=None)
def _consensus():
    c = oi.g14()["consensus"]
    c.setflags(write=False)
    return c


def _read(rng, d, n_lead, n_tail, emb=True, tail_len=None, dwell=None, tail_dwell=None):
    """levels (lead, consensus or noise, tail) x 12 + 85 pA, repeated by their dwell times, plus white noise -> float32.
    ``tail_len``: the tail's samples cut to exactly this many; ``dwell`` / ``tail_dwell``: (lo, hi) instead of 2 d + 2 .. 4 d + 7"""
    cons = _consensus()
    lo, hi = dwell or (2 * d + 2, 4 * d + 8)
    tlo, thi = tail_dwell or (lo, hi)
    if tail_len is not None:
        n_tail = tail_len // tlo + 2
    head = np.concatenate([rng.normal(0, 1, n_lead), cons if emb else rng.normal(0, 1, cons.size)]) * 12.0 + 85.0
    tail = rng.normal(0, 1, n_tail) * 12.0 + 85.0
    x = np.concatenate([np.repeat(head, rng.integers(lo, hi, head.size)), np.repeat(tail, rng.integers(tlo, thi, tail.size))[:tail_len]])
    return (x + rng.normal(0, rng.uniform(0.8, 2.5), x.size)).astype(np.float32)


def _pack(rows, padding):
    """-> (mb (n, stride) float32 with a NaN tail, a_start = padding, a_end = size - padding)"""
    stride = max(r.size for r in rows)
    mb = np.full((len(rows), stride), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        mb[i, : r.size] = r
    return mb, np.full(len(rows), padding, dtype=np.int32), np.array([r.size - padding for r in rows], dtype=np.int32)


def _reference(mb, a_s, a_e, seg, ref, ok=None):
    """dict of the five arrays by the helper's composition through the C statement of the rule, and the seconds it took"""
    t0 = time.perf_counter()
    fpt, dwell, stats, idx, status = oc.refine_batch(mb, a_s, a_e, seg, ref, _consensus(), optimal=True, ok=ok, rule="c")
    want = dict(status=status, fpt=fpt, dwell=dwell, stats=stats, refine_idx=idx)
    rep = (status == 0) | (status == 6)
    assert np.isnan(stats[~rep]).all() and (idx[~rep] == -1).all() and np.isnan(fpt[status != 0]).all()
    for a in want.values():
        a.setflags(write=False)
    return want, time.perf_counter() - t0


def _assert_equal(got, want, what):
    """status, fpt and dwell on every read; stats and refine_idx where the status is 0 or 6, NaN and -1 elsewhere"""
    got = {k: np.asarray(got[k]) for k in NAMES}
    bad = np.flatnonzero(got["status"] != want["status"])
    assert bad.size == 0, (what, "status", bad[:10].tolist(), got["status"][bad[:10]].tolist(), want["status"][bad[:10]].tolist())
    for name in ("fpt", "dwell"):
        assert got[name].shape == want[name].shape, (what, name)
        rows = np.flatnonzero([not same(a, b) for a, b in zip(got[name], want[name])])
        assert rows.size == 0, (what, name, rows[:10].tolist())
    rep = (want["status"] == 0) | (want["status"] == 6)
    for name in ("stats", "refine_idx"):
        rows = np.flatnonzero([not same(a, b) for a, b in zip(got[name][rep], want[name][rep])])
        assert rows.size == 0, (what, name, np.flatnonzero(rep)[rows[:10]].tolist())
    assert np.isnan(got["stats"][~rep]).all() and (got["refine_idx"][~rep] == -1).all(), (what, "stats / refine_idx of unreported reads")


def _params(seg, ref):
    return sig_proc.SegParams(**seg), sig_proc.RefineParams(query=_consensus(), optimal_cpts=True, **ref)


def _blocking(mb, a_s, a_e, seg, ref, ok=None, options=()):
    """sig_proc.fingerprint_refine_batch with context options {option: value} for this call, put back afterwards"""
    hp, hr = _params(seg, ref)
    ctx = _lib.default_context()
    options = dict(options)
    try:
        for o, v in options.items():
            ctx.set_option(o, v)
        return vars(sig_proc.fingerprint_refine_batch(mb, a_s, a_e, hp, hr, success=ok))
    finally:
        for o in options:
            ctx.set_option(o, 0)


class _Launches:
    """counts the launches of fingerprint_refine_optimal_kernel inside the block (WDX_K_REFINE_OPTIMAL of the context's timers)"""

    def __init__(self, ctx):
        self.ctx, self.L, self.n, self.ms = ctx, _lib.load(), None, None

    def __enter__(self):
        _lib.check(self.L.wdx_kernel_time_reset(self.ctx.handle))
        _lib.check(self.L.wdx_kernel_timing(self.ctx.handle, 1))
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                ms, nl = C.c_double(0), C.c_int64(0)
                _lib.check(self.L.wdx_kernel_time(self.ctx.handle, _lib.K_REFINE_OPTIMAL, C.byref(ms), C.byref(nl)))
                self.n, self.ms = nl.value, ms.value
        finally:
            _lib.check(self.L.wdx_kernel_timing(self.ctx.handle, 0))
        return False


# ---- a. more reads than slots ---------------------------------------------------------------------------------------------
TRNA_SEG = dict(padding=100, min_obs_per_base=9, running_stat_width=18, num_events=120, barcode_num_events=25)
TRNA_REF = dict(barcode_segm_events=25, barcode_keep_events=25)
N_SLOTS_BATCH = 420
# the first read of each sequence; its successors in the same workgroup are `slots` and 2 `slots` reads on
AT = dict(global_tail=2, long_lds_tail=4, failed_detection=6, nan_window=8, infeasible=10, outlier=12, infinity=14,
          long_then_short_ok=16)


@functools.lru_cache(maxsize=None)
def slots_batch():
    """420 tRNA-shaped reads, one of them 16 384 samples long with a tail beyond the LDS cap: 199 workgroups, so that the
    workgroup of read i also finishes reads i + 199 and i + 398.  -> dict(mb, a_s, a_e, ok, slots, want, seconds)"""
    rng = np.random.default_rng(4201)
    n, d = N_SLOTS_BATCH, 9
    rows = [_read(rng, d, int(rng.integers(2, 34)), 28, emb=rng.random() > 0.15) for _ in range(n)]
    long_row = _read(rng, d, 8, 40, dwell=(132, 140))[:16384]
    assert long_row.size == 16384
    slots = op.optimal_plan(n, long_row.size, 25)["slots"]
    assert slots <= 209 and n >= 2 * slots + 1 and max(AT.values()) + 2 * slots < n, slots

    def pick(make, status, tail=None):
        """the first of up to 60 candidates that the reference gives this status (and a tail of this many samples)"""
        for _ in range(60):
            x = make()
            st, _, _, _, idx = oc.refine_one(x, 100, x.size - 100, TRNA_SEG, TRNA_REF, _consensus(), optimal=True, rule="c")
            if st == status and (tail is None or tail[0] <= x.size - 36 - int(idx[2]) <= tail[1]):
                return x
        raise AssertionError("no candidate read with status %d and a tail in %s" % (status, tail))

    ordinary = lambda: pick(lambda: _read(rng, d, int(rng.integers(2, 14)), 28), 0)   # noqa: E731
    for first in AT.values():
        for k in (1, 2):
            rows[first + k * slots] = ordinary()
    rows[AT["global_tail"]] = long_row
    rows[AT["long_lds_tail"]] = pick(lambda: _read(rng, d, 8, 0, tail_len=2010, tail_dwell=(60, 80)), 0, (1900, op.LDS_CAP))
    # (a finished read needs its match to end by event 97 of 120, so some 23 events of at least d samples lie behind it: the
    # reference gives status 0 from about 360 samples up.  A tail of 250 .. 300 samples is a consensus outlier -- the dynamic
    # programme and the event means run, stats and refine_idx are reported -- and the shortest finished one follows a long
    # tail in a workgroup of its own)
    short = lambda: _read(rng, d, 1, 0, tail_len=260, tail_dwell=(9, 11))   # noqa: E731
    rows[AT["long_lds_tail"] + slots] = pick(short, 6, (250, 300))
    rows[AT["long_then_short_ok"]] = pick(lambda: _read(rng, d, 8, 0, tail_len=2010, tail_dwell=(60, 80)), 0, (1900, op.LDS_CAP))
    rows[AT["long_then_short_ok"] + slots] = pick(short, 0, (234, 420))
    rows[AT["infeasible"]] = pick(lambda: _read(rng, d, 8, 0, tail_len=40), 3)
    rows[AT["outlier"]] = pick(lambda: _read(rng, d, 34, 28), 6)
    rows[AT["infinity"]] = ordinary()
    for first in ("failed_detection", "nan_window"):
        rows[AT[first]] = ordinary()
    mb, a_s, a_e = _pack(rows, 100)
    ok = np.ones(n, dtype=np.uint8)
    ok[AT["failed_detection"]] = 0
    mb[AT["nan_window"], 1500:1503] = np.nan
    mb[AT["infinity"] + slots, 2000] = np.inf
    want, seconds = _reference(mb, a_s, a_e, TRNA_SEG, TRNA_REF, ok)
    for a in (mb, a_s, a_e, ok):
        a.setflags(write=False)
    return dict(mb=mb, a_s=a_s, a_e=a_e, ok=ok, slots=slots, want=want, seconds=seconds)


def _tail_samples(b, i):
    """N of read i by the reference's barcode start: the window's samples - 2 W - sig_barcode_start (W = 18 here)"""
    return int(b["a_e"][i]) + 100 - (int(b["a_s"][i]) - 100) - 36 - int(b["want"]["refine_idx"][i, 2])


def test_the_slots_batch_is_what_it_claims_by_the_reference_alone():
    """what the reads of `slots_batch` are for, asserted from the reference's own output before any device run is judged"""
    b = slots_batch()
    st, s = b["want"]["status"], b["slots"]
    assert s == 199 and b["mb"].shape[1] == 16384
    assert st[AT["global_tail"]] == 0 and _tail_samples(b, AT["global_tail"]) > op.LDS_CAP
    assert st[AT["long_lds_tail"]] == 0 and 1900 <= _tail_samples(b, AT["long_lds_tail"]) <= op.LDS_CAP
    assert st[AT["long_lds_tail"] + s] == 6 and 250 <= _tail_samples(b, AT["long_lds_tail"] + s) <= 300
    assert st[AT["long_then_short_ok"]] == 0 and 1900 <= _tail_samples(b, AT["long_then_short_ok"]) <= op.LDS_CAP
    assert st[AT["long_then_short_ok"] + s] == 0 and 234 <= _tail_samples(b, AT["long_then_short_ok"] + s) <= 420
    assert st[AT["failed_detection"]] == 1
    assert st[AT["nan_window"]] == 5
    # (one infinity leaves median and MAD finite: the sample is clipped to the upper bound like any spike and the read finishes)
    assert np.isinf(b["mb"][AT["infinity"] + s, 2000]) and st[AT["infinity"] + s] == 0
    assert st[AT["infeasible"]] == 3 and st[AT["outlier"]] == 6 and st[AT["infinity"]] == 0
    for first in AT.values():      # every successor in the same workgroup is an ordinary finished read
        for k in (1, 2):
            if (first, k) != (AT["long_lds_tail"], 1):
                assert st[first + k * s] == 0, (first, k, st[first + k * s])
    # (a lead of 2 .. 33 levels against ub_start = 18 and 15 % of the reads without the consensus: some 45 % finish)
    assert (st == 0).sum() >= 150 and (st == 6).sum() >= 100, np.bincount(st, minlength=8)
    print("reference: %.2f s for %d reads, status counts %s" % (b["seconds"], st.size, np.bincount(st, minlength=8).tolist()))


@pytest.mark.parametrize("entry", ["blocking", "device-minibatch", "device-packed"])
def test_more_reads_than_slots(entry):
    """420 reads on 199 workgroups: each finishes two or three reads, and the sequences of `AT` -- a global-memory tail before
    LDS tails, a long LDS tail before a short one, a failed detection, a NaN window, an infeasible tail, an outlier and an
    infinite sample before or between finished reads -- meet in one workgroup.  One launch per call, whichever entry."""
    b = slots_batch()
    hp, hr = _params(TRNA_SEG, TRNA_REF)
    if entry == "blocking":
        with _Launches(_lib.default_context()) as t:
            got = vars(sig_proc.fingerprint_refine_batch(b["mb"], b["a_s"], b["a_e"], hp, hr, success=b["ok"]))
    else:
        import torch

        from warpdemux_amd.engine import DemuxEngine

        d = lambda a: torch.from_numpy(np.array(a)).cuda()   # noqa: E731
        lens = (b["a_e"] + 100).astype(np.int64)
        eng = DemuxEngine(np.zeros((2, 25)), 15, 0.1, hp)
        try:
            with _Launches(eng.ctx) as t:
                if entry == "device-minibatch":
                    out = eng.fingerprint_refine(d(b["mb"]), d(b["a_s"]), d(b["a_e"]), hr, stride=b["mb"].shape[1],
                                                 max_len=int(lens.max()), ok=d(b["ok"]))
                else:
                    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                    packed = np.concatenate([b["mb"][i, : lens[i]] for i in range(lens.size)])
                    out = eng.fingerprint_refine(d(packed), d(b["a_s"]), d(b["a_e"]), hr, offsets=d(off), max_len=int(lens.max()),
                                                 ok=d(b["ok"]))
                torch.cuda.synchronize()
            fpt, dwell, stats, idx, status = (x.cpu().numpy() for x in out)
            got = dict(status=status, fpt=fpt, dwell=dwell, stats=stats, refine_idx=idx)
        finally:
            eng.close()
    _assert_equal(got, b["want"], entry)
    assert t.n == 1 and t.ms > 0, (entry, t.n, t.ms)


# ---- b. behind every adapter-segmenting kernel at batch size --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_batch():
    """700 reads shaped as test_gpu_refine.py's batch behind the fast kernels; the long tails (every ninth read, 70 .. 110
    events) have dwell times of 12 .. 15 samples instead of 12 .. 49, which keeps the reference affordable"""
    rng = np.random.default_rng(77)
    n = 700
    rows = []
    for i in range(n):
        n_lead = int(rng.integers(2, 34))
        long_tail = i % 9 == 0
        x = _read(rng, 9, n_lead, int(rng.integers(70, 110)) if long_tail else 30, emb=rng.random() > 0.1, dwell=(12, 50),
                  tail_dwell=(12, 16) if long_tail else None)[:8100]
        if i % 50 == 7:
            x = x[: int(rng.integers(1900, 2150))]   # a window too short for the configured width: the parameters shrink
        rows.append(x)
    mb, a_s, a_e = _pack(rows, 100)
    ok = np.ones(n, dtype=np.uint8)
    ok[3] = 0
    mb[5, 1500:1503] = np.nan
    mb[6, 3000] = np.inf
    want, seconds = _reference(mb, a_s, a_e, TRNA_SEG, TRNA_REF, ok)
    for a in (mb, a_s, a_e, ok):
        a.setflags(write=False)
    return dict(mb=mb, a_s=a_s, a_e=a_e, ok=ok, want=want, seconds=seconds)


@pytest.mark.parametrize("path", ["as-planned", "exact-kernel", "three-slices"])
def test_behind_every_adapter_segmenting_kernel_at_batch_size(path):
    """The option on behind the launch chain (fast main, list, retry and split-tail kernels, the exact kernel for what they
    decline), behind the exact kernel alone (WDX_OPT_EXACT_PATH) and behind a chain cut into three launch slices
    (WDX_OPT_MAX_LAUNCH_SLICE = 234): fingerprint_refine_match_wave_kernel matches every record, the optimal kernel finishes
    them -- the reference's bits each time.  At this window length the plan gives 402 slots, so workgroups finish second reads
    here too.  CPU time of the reference for the 700 reads, measured once on the build host: 9.2 s (4.2 s for the whole first
    case on the GPU host; the other two share the reference)."""
    b = chain_batch()
    st = b["want"]["status"]
    assert (st == 0).sum() >= 250 and (st == 6).sum() >= 50 and st[3] == 1, np.bincount(st, minlength=8)
    options = {"as-planned": {}, "exact-kernel": {_lib.OPT_EXACT_PATH: 1}, "three-slices": {_lib.OPT_MAX_LAUNCH_SLICE: 234}}[path]
    got = _blocking(b["mb"], b["a_s"], b["a_e"], TRNA_SEG, TRNA_REF, b["ok"], options)
    _assert_equal(got, b["want"], path)
    print("reference: %.2f s for %d reads, status counts %s" % (b["seconds"], st.size, np.bincount(st, minlength=8).tolist()))


# ---- c. the parameter domain of the whole-read kernel ----------------------------------------------------------------------
#          w   d    E    B   K  norm      padding  events (dwell lo, hi) or None = 2 d + 2 .. 4 d + 7
POINTS = [(12, 6, 110, 10, 10, "mean", 0, None),        # window_stats<12>
          (18, 9, 120, 25, 26, "median", 100, None),    # K = B + 1, the most the branch can give
          (18, 9, 120, 25, 27, "mean", 100, None),      # K = B + 2: every matched read "unknown", stats NaN, idx -1
          (30, 15, 120, 12, 5, "mean", 20, None),       # general loop, K well below B
          (6, 3, 100, 40, 40, "mean", 0, None),         # small W, tiles of 250
          (24, 1, 120, 60, 40, "median", 0, None),      # m = 1
          (18, 2, 120, 253, 30, "mean", 0, None),       # B at its cap (tails of about 80 short events)
          (64, 9, 60, 8, 8, "mean", 0, (150, 201))]     # W = kMaxW, tiles of 192
N_POINT = 48


@functools.lru_cache(maxsize=None)
def point_batch(k):
    w, d, E, B, K, norm, padding, dwell = POINTS[k]
    rng = np.random.default_rng(9000 + k)
    rows = []
    for i in range(N_POINT):
        n_tail = 80 if B == 253 else (12 if w == 64 else max(28, B + 6))
        # (E = 60 at W = 64: the window holds the consensus and a tail, and no lead to speak of)
        x = _read(rng, d, int(rng.integers(0, 3)) if E < 84 else int(rng.integers(2, 20)), n_tail, emb=rng.random() > 0.1,
                  dwell=dwell or ((6, 14) if B == 253 else None))
        if i in (5, 27):                  # the consensus in events shorter than a window, a long tail: a match that ends early
            x = _read(rng, d, 0, 110, dwell=(4, 7), tail_dwell=dwell or (2 * d + 2, 4 * d + 8))
        x = x[:16384]                     # (WDX_MAX_ADAPTER_SAMPLES: the W = 64 point's reads are about that long)
        if i % 11 == 10:
            x = x[: int(0.8 * E * w)]     # the width shrinks: W = rint(n / E) < w
        rows.append(x)
    mb, a_s, a_e = _pack(rows, padding)
    if padding:
        a_s[[4, 15, 26, 37]] = [0, padding // 2, 1, padding - 1]     # a_start < padding: the window starts at the row's start
    seg = dict(padding=padding, min_obs_per_base=d, running_stat_width=w, num_events=E, seg_norm=norm, barcode_num_events=K)
    ref = dict(subseq_norm=norm, psi=(5, 0, 40, 0), ub_start=E, lb_end=40, ub_end=E + 1, barcode_segm_events=B, barcode_keep_events=K)
    want, seconds = _reference(mb, a_s, a_e, seg, ref)
    for a in (mb, a_s, a_e):
        a.setflags(write=False)
    return dict(mb=mb, a_s=a_s, a_e=a_e, seg=seg, ref=ref, want=want, seconds=seconds)


@pytest.mark.parametrize("k", range(len(POINTS)), ids=["w%d-d%d-E%d-B%d-K%d-%s-pad%d" % p[:7] for p in POINTS])
def test_parameter_domain_of_the_whole_read_kernel(k):
    """One point of POINTS, 48 reads, as the plan decides and with the launch chain requested (WDX_OPT_FAST_CHAIN_MIN_READS =
    1; where the fast kernels do not take the width the request changes nothing, and must not)."""
    b = point_batch(k)
    st = b["want"]["status"]
    B, K = POINTS[k][3], POINTS[k][4]
    if K == B + 2:
        assert set(st.tolist()) <= {3, 5, 6} and (st == 5).sum() >= N_POINT // 2, np.bincount(st, minlength=8)
    else:
        assert (st == 0).sum() >= N_POINT // 2, np.bincount(st, minlength=8)
    for what, options in (("as planned", {}), ("chain requested", {_lib.OPT_FAST_CHAIN_MIN_READS: 1})):
        _assert_equal(_blocking(b["mb"], b["a_s"], b["a_e"], b["seg"], b["ref"], None, options), b["want"], (POINTS[k], what))
    print("reference: %.2f s, status counts %s" % (b["seconds"], np.bincount(st, minlength=8).tolist()))


def test_parameter_points_reach_every_status_of_the_branch():
    seen = set()
    for k in range(len(POINTS)):
        seen |= set(point_batch(k)["want"]["status"].tolist())
    assert {0, 3, 5, 6} <= seen, seen


# ---- d. tile ends of the score tail ----------------------------------------------------------------------------------------
N_TILE = 18
TILE_SEG = {18: dict(TRNA_SEG), 12: dict(padding=100, min_obs_per_base=6, running_stat_width=12, num_events=110, barcode_num_events=10)}
TILE_REF = {18: dict(TRNA_REF), 12: dict(barcode_segm_events=10, barcode_keep_events=10)}


@functools.lru_cache(maxsize=None)
def tile_batch(w):
    """18 reads whose a_end is shortened until the tail of the score curve, N = n - 2 W - sig_barcode_start by the reference,
    ends one position before, at and one position behind a tile end of the kernel (tiles of TP = 256 - W positions): read i
    aims at N = (TP - 1, 0, 1)[i % 3] (mod TP).  Shortening the window can move the match; then once more."""
    TP, d = 256 - w, w // 2
    seg, ref = TILE_SEG[w], TILE_REF[w]
    rng = np.random.default_rng(1800 + w)
    rows = [_read(rng, d, int(rng.integers(2, 17)), 30) for _ in range(N_TILE)]
    mb, a_s, a_e = _pack(rows, 100)
    target = np.array([(TP - 1, 0, 1)[i % 3] for i in range(N_TILE)])
    tail = lambda want: (a_e + 100) - (a_s - 100) - 2 * w - want["refine_idx"][:, 2]   # noqa: E731
    want, seconds = _reference(mb, a_s, a_e, seg, ref)
    for _ in range(2):                # re-evaluated once, or twice where the shorter window moved the match
        rep = (want["status"] == 0) | (want["status"] == 6)
        off = np.where(rep, (tail(want) - target) % TP, 0)
        if not off.any():
            break
        a_e = (a_e - off).astype(np.int32)
        want, s = _reference(mb, a_s, a_e, seg, ref)
        seconds += s
    on_target = (tail(want) - target) % TP == 0
    for a in (mb, a_s, a_e):
        a.setflags(write=False)
    return dict(mb=mb, a_s=a_s, a_e=a_e, seg=seg, ref=ref, want=want, seconds=seconds, on_target=on_target)


@pytest.mark.parametrize("w", [18, 12])
def test_tails_that_end_around_a_tile_end(w):
    b = tile_batch(w)
    st = b["want"]["status"]
    hit = (st == 0) & b["on_target"]
    for j, name in enumerate(("TP - 1", "0", "1")):
        assert hit[j::3].sum() >= 2, ("N = %s (mod TP): too few finished reads by the reference" % name, st[j::3], b["on_target"][j::3])
    _assert_equal(_blocking(b["mb"], b["a_s"], b["a_e"], b["seg"], b["ref"]), b["want"], "w = %d" % w)
    print("reference: %.2f s, reads on target %s" % (b["seconds"], [int(hit[j::3].sum()) for j in range(3)]))
