"""``long_windows=True`` on the consensus-refinement branch (WDX_OPT_LONG_REFINE_WINDOWS): adapter windows of 16 385 .. 65 536
samples are segmented, matched against the consensus and their barcode tail segmented again by the refining long form of the
exact kernel (fingerprint_long_refine_kernel: samples and score curve in the workgroup's HBM slot, the tail in place at
sig_barcode_start) -- bit for bit what the reference returns (fixture g13) and what the CPU oracle, which has no window limit,
returns; with the option off nothing changes: such a window is status 5 and every other read keeps its bytes.  The edge
batch of tests/helpers/refine_long_inputs.py under three normalisation pairs, more reads than the kernel has slots, both
dispatch routes, every way in (float32 and int16), and the option's values."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import boost_ref, refine_inputs as ri, refine_long_inputs as rl
from warpdemux_amd import _lib, live, models, pipeline, sig_proc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("status", "fpt", "dwell", "stats", "refine_idx")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _hp(clip64=False, **kw):
    return sig_proc.SegParams(clip_bounds="float64" if clip64 else "float32", **{**dict(barcode_num_events=rl.K, **ri.SEG), **kw})


def _hr(**kw):
    return sig_proc.RefineParams(query=ri.consensus(), **{**ri.REF, **kw})


def _assert_batch(got, want, where=""):
    """got: a FingerprintBatch or a dict of its arrays; want: the oracle's (fpt, dwell, stats, idx, status)"""
    g = got if isinstance(got, dict) else vars(got)
    fpt, dwell, stats, idx, status = want
    assert _same(g["status"], status), f"{where} status: {g['status']} != {status}"
    bad = np.flatnonzero((g["fpt"].view(np.uint64) != fpt.view(np.uint64)).any(axis=1))
    assert _same(g["fpt"], fpt), f"{where} fpt: reads {bad}"
    assert _same(g["dwell"], dwell), f"{where} dwell"
    assert _same(g["stats"], stats), f"{where} stats"
    assert _same(g["refine_idx"], idx), f"{where} refine_idx: {g['refine_idx'].tolist()} != {idx.tolist()}"


# ---- 1. the reference's own values ------------------------------------------------------------------------------------
def test_g13_the_references_values_bit_for_bit():
    g = rl.g13()
    for k in range(int(g["n"])):
        seg, ref, clip64 = rl.params_from(g, k)
        tag = str(g[f"tag_{k}"])
        a_s, a_e = (int(v) for v in g[f"args_{k}"])
        fb = sig_proc.fingerprint_refine_batch(g[f"row_{k}"].reshape(1, -1), [a_s], [a_e], _hp(clip64, **seg),
                                               _hr(**ref), long_windows=True)
        st = int(g[f"status_{k}"])
        assert int(fb.status[0]) == st, f"case {k} ({tag}): status {fb.status[0]} != {st}"
        assert _same(fb.fpt[0], g[f"fpt_{k}"]), f"case {k} ({tag}) fpt"
        assert _same(fb.dwell[0], g[f"dwell_{k}"]), f"case {k} ({tag}) dwell"
        assert _same(fb.stats[0], g[f"stats_{k}"]), f"case {k} ({tag}) stats"
        assert _same(fb.refine_idx[0], g[f"idx_{k}"].astype(np.int32)), f"case {k} ({tag}) refine_idx"
    assert not _lib.default_context().long_refine_windows     # the call put the option back


# ---- 2. / 3. the edges, option on and off -----------------------------------------------------------------------------
EDGE_CASES = {
    "seg-mean": dict(seg={}, ref={}),
    "seg-median": dict(seg=dict(seg_norm="median"), ref={}),
    "subseq-median": dict(seg={}, ref=dict(subseq_norm="median")),
}


@functools.lru_cache(maxsize=None)
def _edge_runs(case):
    """(oracle as the engine reports it, option on, option off) of the edge batch under one configuration"""
    c = EDGE_CASES[case]
    b = rl.edge_batch()
    want = b["want"] if case == "seg-mean" else rl.oracle(b, seg=rl.seg_params(**c["seg"]), ref=rl.refine_params(**c["ref"]))
    args = (b["rows"], b["a_s"], b["a_e"], _hp(**c["seg"]), _hr(**c["ref"]))
    on = sig_proc.fingerprint_refine_batch(*args, success=b["ok"], long_windows=True)
    off = sig_proc.fingerprint_refine_batch(*args, success=b["ok"])
    return rl.expected(want, b["win"]), on, off


@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_edges_option_on_equals_the_oracle(case):
    want, on, _off = _edge_runs(case)
    b = rl.edge_batch()
    _assert_batch(on, want, case)
    st = want[4]
    long = (b["win"] > rl.CAP) & (b["win"] <= rl.LONG_CAP)
    assert (long & (st == 0)).sum() >= 6 and (long & (st == 6)).sum() >= 2, st     # the long kernel did refine
    assert st[6] == 5 and b["win"][6] == rl.LONG_CAP + 1                          # 65 537 samples: "unknown"
    assert st[rl.I_FEW_PEAKS] == 3 and st[rl.I_FLAT_TAIL] == 3 and st[rl.I_DEAD] == 1


@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_edges_option_off_changes_nothing_else(case):
    _want, on, off = _edge_runs(case)
    b = rl.edge_batch()
    long = (b["win"] > rl.CAP) & (b["ok"] != 0)
    assert long.sum() == 15
    assert (off.status[long] == 5).all() and np.isnan(off.fpt[long]).all() and not off.dwell[long].any()
    assert np.isnan(off.stats[long]).all() and (off.refine_idx[long] == -1).all()
    for name in NAMES:
        assert _same(getattr(off, name)[~long], getattr(on, name)[~long]), f"{case}: {name}"
    assert (off.status[~long] != 5).all()


# ---- 4. more reads than slots, both dispatch routes ---------------------------------------------------------------------
def test_more_long_windows_than_slots():
    """40 windows of 16 400 .. 17 400 samples in one call: the kernel's 16 workgroups come round to their slots again"""
    rng = np.random.default_rng(43)
    lens = rng.integers(16400, 17401, 40)
    mb = rl.minibatch([rl.read(rng, int(m), embed=i % 7 != 3) for i, m in enumerate(lens)])
    b = dict(rows=mb, a_s=np.full(40, rl.PADDING, np.int32), a_e=(lens - rl.PADDING).astype(np.int32), ok=None)
    want = rl.oracle(b)
    assert (want[4] == 0).sum() >= 25 and (want[4] == 6).sum() >= 4, want[4]
    _assert_batch(sig_proc.fingerprint_refine_batch(mb, b["a_s"], b["a_e"], _hp(), _hr(), long_windows=True), want, "slots")


@functools.lru_cache(maxsize=None)
def _route_batch():
    """2 100 reads -- from 2 048 on a batch takes the launch chain -- of which 8 are long (tests/helpers/refine_inputs.py's
    reads around them), and the oracle on them"""
    n, at = 2100, (0, 5, 300, 777, 1024, 1500, 2047, 2099)
    base = ri.batch(77, n=n)
    lens = (16385, 16448, 17000, 18000, 16600, 19000, 16449, 20000)
    rng = np.random.default_rng(44)
    mb = np.full((n, 20000), np.nan, dtype=np.float32)
    mb[:, : base["rows"].shape[1]] = base["rows"]
    a_s, a_e = base["a_s"].copy(), base["a_e"].copy()
    for i, m in zip(at, lens):
        mb[i] = np.nan
        mb[i, :m] = rl.read(rng, m)
        a_s[i], a_e[i] = rl.PADDING, m - rl.PADDING
    ok = base["ok"].copy()
    ok[list(at)] = 1
    b = dict(rows=mb, a_s=a_s, a_e=a_e, ok=ok)
    want = rl.oracle(b)
    assert (want[4][list(at)] == 0).sum() >= 6 and (want[4] == 0).sum() >= n * 40 // 96, want[4][list(at)]   # (refine_inputs.check_kinds' share)
    return b, want, at


@pytest.mark.parametrize("route", ["chain", "single-launch"])
def test_both_routes_hand_long_windows_to_the_refining_long_kernel(route, capfd):
    """the launch chain (the default for 2 100 reads) and the exact kernel's single launch (WDX_OPT_EXACT_PATH) each end in
    the same step behind launch_fp_big; which route ran is read from WDX_OPT_DEBUG_OCCUPANCY's report of the chain"""
    b, want, at = _route_batch()
    ctx = _lib.default_context()
    ctx.set_option(_lib.OPT_DEBUG_OCCUPANCY, 1)
    if route == "single-launch":
        ctx.set_option(_lib.OPT_EXACT_PATH, 1)
    try:
        capfd.readouterr()
        on = sig_proc.fingerprint_refine_batch(b["rows"], b["a_s"], b["a_e"], _hp(), _hr(), success=b["ok"], long_windows=True)
        err = capfd.readouterr().err
        off = sig_proc.fingerprint_refine_batch(b["rows"], b["a_s"], b["a_e"], _hp(), _hr(), success=b["ok"])
    finally:
        ctx.set_option(_lib.OPT_DEBUG_OCCUPANCY, 0)
        ctx.set_option(_lib.OPT_EXACT_PATH, 0)
    assert ("[wdx] fast kernel capF=" in err) == (route == "chain"), err[-1500:]
    _assert_batch(on, want, route)
    assert (off.status[list(at)] == 5).all() and (off.refine_idx[list(at)] == -1).all()
    rest = np.setdiff1d(np.arange(off.status.size), at)
    for name in NAMES:
        assert _same(getattr(off, name)[rest], getattr(on, name)[rest]), f"{route}: {name}"


# ---- 5. every way in ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ways():
    """the 12 reads, and the module-level call's result on their float32 rows (held against the oracle by the first test)"""
    b = rl.ways_batch()
    base = sig_proc.fingerprint_refine_batch(b["rows"], b["a_s"], b["a_e"], _hp(), _hr(), success=b["ok"], long_windows=True)
    for name in NAMES:
        getattr(base, name).setflags(write=False)
    return b, base


def _assert_way(got, where, names=NAMES):
    _b, base = _ways()
    g = got if isinstance(got, dict) else vars(got)
    for name in names:
        assert _same(g[name], getattr(base, name)), f"{where}: {name}"


@functools.lru_cache(maxsize=None)
def _boost_model():
    m = boost_ref.random_model(65, 6, 4, rl.K, seed=81)
    trees = [(f, bd, [False] * len(f), lv) for f, bd, lv in m.trees]
    return models.Fpt_Boost(trees, m.n_features, m.scale, m.bias, {0: 7, 1: 1, 2: 10, 3: 4}, np.array([0.05, 0.2, 0.1, 0.3]))


def test_ways_the_batch_call_equals_the_oracle():
    b, base = _ways()
    _assert_batch(base, b["want"], "fingerprint_refine_batch")
    assert (base.status[b["long"]] == 0).sum() >= 5
    off = sig_proc.fingerprint_refine_batch(b["rows"], b["a_s"], b["a_e"], _hp(), _hr(), success=b["ok"])
    assert (off.status[b["long"]] == 5).all() and _same(off.fpt[~b["long"]], base.fpt[~b["long"]])


def test_ways_engine_demux_refine_and_demux_boost():
    import torch

    from warpdemux_amd.engine import DemuxEngine
    b, base = _ways()
    good = base.status == 0
    refs = np.ascontiguousarray(base.fpt[good][:6])
    eng = DemuxEngine(refs, 15, 0.1, _hp(), long_windows=True)
    d = lambda a: torch.from_numpy(np.array(a)).to(eng.tdev)  # noqa: E731  (a copy: the batch's arrays are read-only)
    try:
        rows, stride = d(b["rows"]), b["rows"].shape[1]
        res, dwell, stats, idx = eng.demux_refine(rows, d(b["a_s"]), d(b["a_e"]), _hr(), stride=stride, max_len=stride, ok=d(b["ok"]))
        torch.cuda.synchronize()
        _assert_way(dict(status=res.status.cpu().numpy(), fpt=res.fpt.cpu().numpy(), dwell=dwell.cpu().numpy(),
                         stats=stats.cpu().numpy(), refine_idx=idx.cpu().numpy()), "demux_refine")
        call = res.call.cpu().numpy()
        assert (call[good] >= 0).all() and (call[~good] == -1).all() and (call[np.flatnonzero(good)[:6]] == np.arange(6)).all()
        fpt, dwell, stats, idx, status = eng.fingerprint_refine(rows, d(b["a_s"]), d(b["a_e"]), _hr(), stride=stride,
                                                                max_len=stride, ok=d(b["ok"]))
        torch.cuda.synchronize()
        _assert_way(dict(status=status.cpu().numpy(), fpt=fpt.cpu().numpy(), dwell=dwell.cpu().numpy(),
                         stats=stats.cpu().numpy(), refine_idx=idx.cpu().numpy()), "fingerprint_refine")
        eng.set_boost(_boost_model())
        prob, pred, conf, status, idx, fpt, _raw = eng.demux_boost(rows, d(b["a_s"]), d(b["a_e"]), _hr(), stride=stride,
                                                                   max_len=stride, ok=d(b["ok"]), want_fpt=True)
        torch.cuda.synchronize()
        _assert_way(dict(status=status.cpu().numpy(), fpt=fpt.cpu().numpy(), refine_idx=idx.cpu().numpy()), "demux_boost",
                    ("status", "fpt", "refine_idx"))
        assert np.isfinite(prob.cpu().numpy()[good]).all() and (pred.cpu().numpy()[~good] == -1).all()
    finally:
        eng.close()


def test_ways_minibatch_pipeline():
    b, _base = _ways()
    pl = pipeline.MinibatchPipeline(None, params=_hp(), refine=_hr(), long_windows=True)
    try:
        pinned = pipeline.pinned_empty(b["rows"].shape, np.float32)
        pinned[:] = b["rows"]
        pl.submit(0, pinned, b["a_s"], b["a_e"], success=b["ok"])
        pl.submit_adc(1, b["adc"], b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"], success=b["ok"])
        r0, r1 = pl.wait(0), pl.wait(1)
        pl.submit(0, b["rows"], b["a_s"], b["a_e"], success=b["ok"])     # pageable
        r2 = pl.wait(0)
    finally:
        pl.close()
    for r, name in ((r0, "submit (page-locked)"), (r1, "submit_adc"), (r2, "submit (pageable)")):
        _assert_way(r.fingerprints, name)


def test_ways_live_ticks():
    b, base = _ways()
    kw = dict(want_fpt=True, want_dwell=True, want_stats=True, want_refine_idx=True)
    stride = b["rows"].shape[1]
    rows = [np.ascontiguousarray(b["rows"][i, : min(int(b["row_len"][i]) + 200, stride)]) for i in range(12)]   # (with NaN tail)
    adc_rows = [np.ascontiguousarray(b["adc"][i, : b["row_len"][i]]) for i in range(12)]
    ld = live.LiveDemux(model=_boost_model(), params=_hp(), refine=_hr(), max_reads=12, max_samples=2000, long_windows=True)
    try:
        t = ld.tick(rows, b["a_s"], b["a_e"], success=b["ok"], **kw)
        ta = ld.tick_adc(adc_rows, b["offset"], b["scale"], b["a_s"], b["a_e"], success=b["ok"], **kw)
    finally:
        ld.close()
    _assert_way(t, "LiveDemux.tick")
    _assert_way(ta, "LiveDemux.tick_adc")
    assert _same(t.pred, ta.pred) and (t.pred[base.status != 0] == -1).all()
    # without the option an int16 tick reports the long windows (its staging cuts them one sample beyond the default cap)
    ld = live.LiveDemux(model=_boost_model(), params=_hp(), refine=_hr(), max_reads=12, max_samples=2000)
    try:
        t0 = ld.tick_adc(adc_rows, b["offset"], b["scale"], b["a_s"], b["a_e"], success=b["ok"], **kw)
    finally:
        ld.close()
    long = b["long"]
    assert (t0.status[long] == 5).all()
    for name in NAMES:
        assert _same(getattr(t0, name)[~long], getattr(ta, name)[~long]), name


def test_ways_feeder_worker(tmp_path):
    out = str(tmp_path / "feeder.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "feeder_refine_long_check.py"), out],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = np.load(out)
    for kind in ("f32", "i16"):
        _assert_way({name: got[f"{kind}_{name}"] for name in NAMES}, f"Feeder ({kind})")


# ---- 6. the option's values -----------------------------------------------------------------------------------------------
def test_the_option_takes_0_and_1_only():
    ctx = _lib.Context(0)
    try:
        for bad in (2, -1):
            with pytest.raises(ValueError, match="WDX_OPT_LONG_REFINE_WINDOWS"):
                ctx.set_option(_lib.OPT_LONG_REFINE_WINDOWS, bad)
        assert not ctx.long_refine_windows
        ctx.set_option(_lib.OPT_LONG_REFINE_WINDOWS, 1)
        ctx.set_option(_lib.OPT_LONG_REFINE_WINDOWS, 0)
    finally:
        ctx.close()
