"""``long_windows=True`` (WDX_OPT_LONG_WINDOWS): adapter windows of 16 385 .. 65 536 samples are fingerprinted by the long form
of the exact kernel (fingerprint_long_kernel: samples and score curve in the workgroup's HBM slot) -- bit for bit what the
reference returns (fixture g12) and what the CPU oracle, which has no window limit, returns; with the option off nothing
changes: such a window is status 5 and every other read keeps its bytes.  Both dispatch routes (the exact-only route of small
batches, the launch chain of large ones), more reads than the kernel has slots, every way in, and the refusals (beyond
65 536 samples, the refinement branch, a value other than 0 / 1)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import long_inputs as li
from oracle import wdx_oracle as orc
from warpdemux_amd import _lib, live, pipeline, sig_proc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _params(g, k):
    pad, sig_norm, d, w, E, acc, seg_norm, K = (int(v) for v in g[f"params_{k}"])
    inv = {0: "none", 1: "mean", 2: "median"}
    kw = dict(padding=pad, sig_norm=inv[sig_norm], outlier_thresh=float(g[f"thresh_{k}"]), min_obs_per_base=d,
              running_stat_width=w, num_events=E, accept_less_cpts=bool(acc), seg_norm=inv[seg_norm], barcode_num_events=K)
    c64 = bool(int(g[f"clip64_{k}"]))
    return sig_proc.SegParams(clip_bounds="float64" if c64 else "float32", **kw)


def _pair(clip64=False, **kw):
    """the engine's and the oracle's parameters of one configuration"""
    return (sig_proc.SegParams(clip_bounds="float64" if clip64 else "float32", **kw), orc.SegParams(clip_bounds_f64=clip64, **kw))


def _assert_batch(fb, want, where=""):
    fpt, dwell, stats, status = want
    assert _same(fb.status, status), f"{where} status: {fb.status} != {status}"
    assert _same(fb.fpt, fpt), f"{where} fpt: reads {np.flatnonzero((fb.fpt.view(np.uint64) != fpt.view(np.uint64)).any(axis=1))}"
    assert _same(fb.dwell, dwell), f"{where} dwell"
    assert _same(fb.stats, stats), f"{where} stats"


# ---- 1. the reference's own values ------------------------------------------------------------------------------------
def test_g12_the_references_values_bit_for_bit():
    g = li.g12()
    tags = set()
    for k in range(int(g["n"])):
        tag = str(g[f"tag_{k}"])
        a_start, a_end, ok = (int(v) for v in g[f"args_{k}"])
        fb = sig_proc.fingerprint_batch(g[f"row_{k}"].reshape(1, -1), [a_start], [a_end], _params(g, k), success=[ok],
                                        long_windows=True)
        st_ref = int(g[f"status_{k}"])
        assert int(fb.status[0]) == st_ref, f"case {k} ({tag}): status {fb.status[0]} != {st_ref}"
        if st_ref == 0:
            assert _same(fb.fpt[0], g[f"fpt_{k}"]), f"case {k} ({tag}) fpt"
            assert _same(fb.dwell[0], g[f"dwell_{k}"]), f"case {k} ({tag}) dwell"
            assert _same(fb.stats[0], g[f"stats_{k}"]), f"case {k} ({tag}) stats"
        else:
            assert np.isnan(fb.fpt[0]).all() and not fb.dwell[0].any()
        tags.add(tag)
    assert {"rna004_16385", "rna002_65536", "trna_65536", "rna002_20000_signorm_mean", "rna002_20000_nan_middle"} <= tags
    assert not _lib.default_context().long_windows     # the call put the option back


# ---- 2. / 3. the edges, option on and off -----------------------------------------------------------------------------
EDGE_CASES = {
    "rna004": dict(triple="rna004"),
    "rna002": dict(triple="rna002"),
    "trna": dict(triple="trna"),
    "rna002-accept-less-clip64": dict(triple="rna002", accept_less_cpts=True, clip64=True, outlier_thresh=2.7),
    "rna004-accept-less": dict(triple="rna004", accept_less_cpts=True),
    "trna-clip64": dict(triple="trna", clip64=True),
}


@functools.lru_cache(maxsize=None)
def _edges():
    b = li.edge_batch()
    for a in b.values():
        a.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _edge_runs(case):
    """(oracle, option on, option off) of the edge batch under one configuration"""
    c = dict(EDGE_CASES[case])
    kw = dict(padding=li.PADDING, barcode_num_events=li.K, **li.TRIPLES[c.pop("triple")])
    clip64 = c.pop("clip64", False)
    p_hip, p_orc = _pair(clip64, **kw, **c)
    b = _edges()
    want = orc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], p_orc, ok=b["ok"])
    on = sig_proc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], p_hip, success=b["ok"], long_windows=True)
    off = sig_proc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], p_hip, success=b["ok"])
    return want, on, off


def test_the_edge_batch_holds_its_edges():
    b = _edges()
    assert tuple(b["win"][: len(li.EDGE_LENGTHS)]) == li.EDGE_LENGTHS and b["win"].size == 26
    assert b["win"][23] == 16600 and b["a_s"][17] < li.PADDING and b["a_s"][18] < li.PADDING and not b["ok"][16]
    assert (b["win"] > li.LONG_CAP).sum() == 2 and ((b["win"] > li.CAP) & (b["win"] <= li.LONG_CAP)).sum() >= 15


@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_edges_option_on_equals_the_oracle(case):
    want, on, _off = _edge_runs(case)
    b = _edges()
    fpt, dwell, stats, status = (a.copy() for a in want)
    beyond = b["win"] > li.LONG_CAP           # the oracle has no limit; the engine's is 65 536 with the option on
    status[beyond], fpt[beyond], dwell[beyond], stats[beyond] = 5, np.nan, 0, np.nan
    _assert_batch(on, (fpt, dwell, stats, status), case)
    long_ok = (b["win"] > li.CAP) & ~beyond & (status == 0)
    assert long_ok.sum() >= 9, status        # the long kernel did produce fingerprints
    assert status[16] == 1 and status[15] != 0 and status[19] != 0
    assert (status[[24, 25]] == (0 if "accept-less" in case else 3)).all(), status[[24, 25]]


@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_edges_option_off_changes_nothing_else(case):
    _want, on, off = _edge_runs(case)
    b = _edges()
    long = (b["win"] > li.CAP) & (b["ok"] != 0)
    assert (off.status[long] == 5).all() and np.isnan(off.fpt[long]).all() and not off.dwell[long].any()
    assert np.isnan(off.stats[long]).all()
    for name in ("status", "fpt", "dwell", "stats"):
        assert _same(getattr(off, name)[~long], getattr(on, name)[~long]), f"{case}: {name}"


# ---- 4. both dispatch routes, more reads than slots ---------------------------------------------------------------------
def test_chain_route_hands_long_windows_to_the_long_kernel():
    """2 108 reads -- from 2 048 on a batch takes the launch chain -- of which 8 are long: they reach the end of the chain
    through the slow list"""
    rng = np.random.default_rng(41)
    n, at = 2108, (0, 5, 300, 777, 1024, 1500, 2047, 2107)
    lens = np.full(n, 1500)
    lens[list(at)] = (16385, 16448, 17000, 18000, 16600, 19000, 16385 + 64, 20000)
    rows = [li.step_row(rng, int(m), 1500 / 135.0) for m in lens]
    mb = li.minibatch(rows)
    a_s, a_e = np.full(n, li.PADDING, np.int32), (lens - li.PADDING).astype(np.int32)
    p_hip, p_orc = _pair(padding=li.PADDING, barcode_num_events=li.K, **li.TRIPLES["rna004"])
    want = orc.fingerprint_batch(mb, a_s, a_e, p_orc)
    assert (want[3][list(at)] == 0).all() and (want[3] == 0).sum() > 2000
    _assert_batch(sig_proc.fingerprint_batch(mb, a_s, a_e, p_hip, long_windows=True), want, "chain")
    off = sig_proc.fingerprint_batch(mb, a_s, a_e, p_hip)
    assert (off.status[list(at)] == 5).all()
    rest = np.setdiff1d(np.arange(n), at)
    assert _same(off.fpt[rest], want[0][rest]) and _same(off.status[rest], want[3][rest])


def test_more_long_windows_than_slots():
    """300 windows of 16 400 .. 16 600 samples on the exact-only route: the kernel's slot loop wraps many times"""
    rng = np.random.default_rng(42)
    lens = rng.integers(16400, 16601, 300)
    mb = li.minibatch([li.step_row(rng, int(m)) for m in lens])
    a_s, a_e = np.full(300, li.PADDING, np.int32), (lens - li.PADDING).astype(np.int32)
    p_hip, p_orc = _pair(padding=li.PADDING, barcode_num_events=li.K, **li.TRIPLES["rna002"])
    want = orc.fingerprint_batch(mb, a_s, a_e, p_orc)
    assert (want[3] == 0).sum() >= 290
    _assert_batch(sig_proc.fingerprint_batch(mb, a_s, a_e, p_hip, long_windows=True), want, "slots")


# ---- 5. every way in ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ways():
    """the 12 reads, the oracle on their float32 rows, the module-level call's result (test 1's call), 10 references"""
    b = li.ways_batch()
    p_hip, p_orc = _pair(**li.WAYS_SEG)
    want = orc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], p_orc, ok=b["ok"])
    base = sig_proc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], p_hip, success=b["ok"], long_windows=True)
    good = np.flatnonzero(want[3] == 0)
    assert good.size >= 9 and want[3][8] == 1 and want[3][10] != 0
    refs = np.ascontiguousarray(np.concatenate([want[0][good], want[0][good[:1]] + 0.25])[:10])
    assert refs.shape == (10, li.K)
    return b, p_hip, want, base, refs


def _assert_way(got_status, got_fpt, where):
    _b, _p, _want, base, _refs = _ways()
    assert _same(got_status, base.status), f"{where}: status {got_status} != {base.status}"
    assert _same(got_fpt, base.fpt), f"{where}: fpt"


def test_ways_the_module_level_call_equals_the_oracle():
    _b, _p, want, base, _refs = _ways()
    _assert_batch(base, want, "fingerprint_batch")


def test_ways_demux_batch_and_its_dtw():
    b, p, want, base, refs = _ways()
    sig_proc.set_references(refs, 15, 0.1)
    db = sig_proc.demux_batch(b["rows"], b["a_s"], b["a_e"], p, success=b["ok"], want_fpt=True, long_windows=True)
    _assert_way(db.status, db.fpt, "demux_batch")
    good = want[3] == 0
    D = orc.dtw_matrix(want[0][good], refs, 15, 0.1)
    assert _same(db.dist[good], D) and np.isnan(db.dist[~good]).all()
    call = np.full(12, -1, np.int32)
    call[good] = np.argmin(D, axis=1)
    assert _same(db.call, call)
    da = sig_proc.demux_batch_adc(b["adc"], b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"], p, success=b["ok"],
                                  want_fpt=True, long_windows=True)
    _assert_way(da.status, da.fpt, "demux_batch_adc")
    assert _same(da.call, call) and _same(da.dist, db.dist)
    off = sig_proc.demux_batch(b["rows"], b["a_s"], b["a_e"], p, success=b["ok"])     # the default: today's behaviour
    long = (want[3] == 0) & (b["a_e"] - b["a_s"] + 2 * li.PADDING > li.CAP)
    assert long.sum() >= 6 and (off.status[long] == 5).all() and (off.call[long] == -1).all()


def test_ways_fingerprint_batch_adc():
    b, p, _want, base, _refs = _ways()
    fa = sig_proc.fingerprint_batch_adc(b["adc"], b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"], p, success=b["ok"],
                                        long_windows=True)
    _assert_way(fa.status, fa.fpt, "fingerprint_batch_adc")
    assert _same(fa.dwell, base.dwell) and _same(fa.stats, base.stats)


def test_ways_minibatch_pipeline():
    b, p, _want, _base, refs = _ways()
    pl = pipeline.MinibatchPipeline(refs, 15, 0.1, p, long_windows=True)
    try:
        pinned = pipeline.pinned_empty(b["rows"].shape, np.float32)
        pinned[:] = b["rows"]
        pl.submit(0, pinned, b["a_s"], b["a_e"], success=b["ok"], want_fpt=True)
        pl.submit_adc(1, b["adc"], b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"], success=b["ok"], want_fpt=True)
        r0, r1 = pl.wait(0), pl.wait(1)
        pl.submit(0, b["rows"], b["a_s"], b["a_e"], success=b["ok"], want_fpt=True)     # pageable
        r2 = pl.wait(0)
    finally:
        pl.ctx.close()
    for r, name in ((r0, "submit (page-locked)"), (r1, "submit_adc"), (r2, "submit (pageable)")):
        _assert_way(r.status, r.fpt, name)
    assert _same(r0.call, r1.call) and _same(r0.call, r2.call)


def test_ways_engine_on_packed_device_rows():
    import torch

    from warpdemux_amd.engine import DemuxEngine
    b, p, _want, base, refs = _ways()
    lens = b["row_len"].astype(np.int64) + 128          # every packed row keeps some of its NaN tail (read 10 looks into it)
    lens = np.minimum(lens, b["rows"].shape[1])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.concatenate([b["rows"][i, : lens[i]] for i in range(12)])
    eng = DemuxEngine(refs, 15, 0.1, p, long_windows=True)
    dev = eng.tdev
    fpt, dwell, stats, status = eng.fingerprint(torch.from_numpy(flat).to(dev), torch.from_numpy(b["a_s"]).to(dev),
                                                torch.from_numpy(b["a_e"]).to(dev), offsets=torch.from_numpy(off).to(dev),
                                                max_len=li.LONG_CAP, ok=torch.from_numpy(b["ok"]).to(dev))
    torch.cuda.synchronize()
    _assert_way(status.cpu().numpy(), fpt.cpu().numpy(), "DemuxEngine.fingerprint")
    assert _same(dwell.cpu().numpy(), base.dwell) and _same(stats.cpu().numpy(), base.stats)
    eng.ctx.close()


def test_ways_live_ticks():
    b, p, _want, _base, refs = _ways()
    ld = live.LiveDemux(refs, 15, 0.1, p, max_reads=12, max_samples=2000, long_windows=True)
    try:
        stride = b["rows"].shape[1]
        rows = [np.ascontiguousarray(b["rows"][i, : min(int(b["row_len"][i]) + 200, stride)]) for i in range(12)]   # (with NaN tail)
        t = ld.tick(rows, b["a_s"], b["a_e"], success=b["ok"], want_fpt=True)
        adc_rows = [np.ascontiguousarray(b["adc"][i, : b["row_len"][i]]) for i in range(12)]
        ta = ld.tick_adc(adc_rows, b["offset"], b["scale"], b["a_s"], b["a_e"], success=b["ok"], want_fpt=True)
    finally:
        ld.close()
    _assert_way(t.status, t.fpt, "LiveDemux.tick")
    _assert_way(ta.status, ta.fpt, "LiveDemux.tick_adc")
    assert _same(t.call, ta.call)
    # without the option an int16 tick reports the long windows (its staging cuts them one sample beyond the default cap)
    ld = live.LiveDemux(refs, 15, 0.1, p, max_reads=12, max_samples=2000)
    try:
        t0 = ld.tick_adc(adc_rows, b["offset"], b["scale"], b["a_s"], b["a_e"], success=b["ok"], want_fpt=True)
    finally:
        ld.close()
    long = (b["a_e"] - b["a_s"] + 2 * li.PADDING > li.CAP) & (b["ok"] != 0)
    assert (t0.status[long] == 5).all() and _same(t0.status[~long], ta.status[~long]) and _same(t0.fpt[~long], ta.fpt[~long])


def test_ways_feeder_worker(tmp_path):
    out = str(tmp_path / "feeder.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "feeder_long_check.py"), out],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = np.load(out)
    _assert_way(got["status"], got["fpt"], "Feeder.fingerprint_batch")
    assert _same(got["demux_status"], _ways()[3].status)
    _b, _p, want, _base, refs = _ways()
    good = want[3] == 0
    call = np.full(12, -1, np.int32)
    call[good] = np.argmin(orc.dtw_matrix(want[0][good], refs, 15, 0.1), axis=1)
    assert _same(got["call"], call)


# ---- 6. the refinement branch keeps the default limit -------------------------------------------------------------------
def test_refinement_does_not_take_long_windows():
    from helpers import refine_inputs as ri

    n = 96                                       # (the size `refine_inputs.check_kinds` speaks about)
    b = ri.batch(101, n=n)                      # (a seed tests/test_gpu_refine_paths.py holds check_kinds on)
    rng = np.random.default_rng(6)
    long_row = li.step_row(rng, 20000)
    mb = np.full((n + 1, 20000), np.nan, dtype=np.float32)
    mb[:n, : b["rows"].shape[1]] = b["rows"]
    mb[n] = long_row
    a_s = np.concatenate([b["a_s"], [li.PADDING]]).astype(np.int32)
    a_e = np.concatenate([b["a_e"], [20000 - li.PADDING]]).astype(np.int32)
    ok = np.concatenate([b["ok"], [1]]).astype(np.uint8)
    p = sig_proc.SegParams(barcode_num_events=25, **ri.SEG)
    rp = sig_proc.RefineParams(query=ri.consensus(), **ri.REF)
    off = sig_proc.fingerprint_refine_batch(mb, a_s, a_e, p, rp, success=ok)
    with _lib.default_context().long_windows_for_call(True):
        on = sig_proc.fingerprint_refine_batch(mb, a_s, a_e, p, rp, success=ok)
    assert on.status[n] == 5 and off.status[n] == 5 and np.isnan(on.fpt[n]).all()
    ri.check_kinds(on.status[:n], with_nan=False)
    for name in ("status", "fpt", "dwell", "stats", "refine_idx"):
        assert _same(getattr(on, name), getattr(off, name)), name
    # the same window on the plain branch of the same context is served
    plain = sig_proc.fingerprint_batch(mb[n:], a_s[n:], a_e[n:], p, long_windows=True)
    assert plain.status[0] == 0


# ---- 7. the option's values -----------------------------------------------------------------------------------------------
def test_the_option_takes_0_and_1_only():
    ctx = _lib.Context(0)
    try:
        for bad in (2, -1, 65536):
            with pytest.raises(ValueError, match="WDX_OPT_LONG_WINDOWS"):
                ctx.set_option(_lib.OPT_LONG_WINDOWS, bad)
        ctx.set_option(_lib.OPT_LONG_WINDOWS, 1)
        ctx.set_option(_lib.OPT_LONG_WINDOWS, 0)
    finally:
        ctx.close()
