"""Optimal change-points of the consensus refinement on the device (WDX_OPT_REFINE_OPTIMAL_CPTS): the dynamic programme
through its kernel-level entry (wdx_selftest_optimal_cpts_dev) against the NumPy restatement -- change-points identical --
and whole reads of fixture g14 (the reference's code around a stand-in for ruptures.KernelCPD) through every way in: every
array bit for bit, NaN by position; no tolerances."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import adc_inputs, boost_ref, optimal_cpts as oc, optimal_inputs as oi
from oracle import wdx_oracle as orc
from warpdemux_amd import _lib, models, pipeline, sig_proc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_CAP = 2047          # kOptLdsCap (wdx_refine_optimal_plan.h): tails whose prefix sums and value rows live in LDS
MAX_BKPS = 253          # the cap of barcode_segm_events
OK, SEGMENT = 0, 3
same = oi.same


def _device_cpts(series, n_bkps, min_size, max_slots=0, max_len=None):
    """(cpts (n, B + 2) int32, status (n,)) of wdx_selftest_optimal_cpts_dev on a list of float64 series"""
    import torch

    n = len(series)
    off = np.concatenate([[0], np.cumsum([len(s) for s in series])]).astype(np.int64)
    x = np.concatenate([np.asarray(s, np.float64) for s in series] + [np.zeros(1)])
    dx, doff = torch.from_numpy(x).cuda(), torch.from_numpy(off).cuda()
    cp = torch.full((n, n_bkps + 2), -7, dtype=torch.int32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ctx = _lib.default_context()
    if max_len is None:
        max_len = max(len(s) for s in series)
    _lib.check(_lib.load().wdx_selftest_optimal_cpts_dev(ctx.handle, C.c_void_p(dx.data_ptr()), C.c_void_p(doff.data_ptr()), n,
                                                         n_bkps, min_size, max_len, max_slots, C.c_void_p(cp.data_ptr()),
                                                         C.c_void_p(st.data_ptr()), None))
    torch.cuda.synchronize()
    return cp.cpu().numpy(), st.cpu().numpy()


def _check(series, n_bkps, min_size, what, **kw):
    cp, st = _device_cpts(series, n_bkps, min_size, **kw)
    n_ok = 0
    for i, s in enumerate(series):
        exp = oc.optimal_cpts(s, n_bkps, min_size)
        if exp is None:
            assert st[i] == SEGMENT and (cp[i] == -1).all(), (what, i, len(s), st[i], cp[i])
        else:
            assert st[i] == OK and cp[i].tolist() == exp.tolist(), (what, i, len(s), st[i], cp[i].tolist(), exp.tolist())
            n_ok += 1
    return n_ok


def _noisy_steps(rng, n, n_steps=6):
    lv = np.repeat(rng.normal(0, 4, n_steps), -(-n // n_steps))[:n]
    return lv + rng.normal(0, 1, n)


def test_kernel_feasibility_edges_and_small_parameters():
    rng = np.random.default_rng(1)
    B, m = 3, 9
    assert _check([_noisy_steps(rng, N) for N in ((B + 1) * m, (B + 1) * m - 1, (B + 1) * m + 1)], B, m, "N around (B+1)m") == 2
    assert _check([_noisy_steps(rng, N) for N in (4, 3, 5, 64, 200)], 3, 1, "m = 1") == 4
    assert _check([_noisy_steps(rng, N) for N in (10, 9, 11, 63, 64, 65, 300)], 1, 5, "B = 1") == 6
    assert _check([_noisy_steps(rng, N, 40) for N in (MAX_BKPS + 1, MAX_BKPS, MAX_BKPS + 2, 600)], MAX_BKPS, 1, "B at its cap") == 3


def test_kernel_wave_and_block_sized_tails():
    rng = np.random.default_rng(2)
    assert _check([_noisy_steps(rng, N) for N in (63, 64, 65, 255, 256, 257)], 4, 6, "N around 64 and 256") == 6


def test_kernel_around_the_lds_cap():
    """LDS form up to kOptLdsCap samples, the global-memory form beyond: the last of the first, the first two of the second"""
    rng = np.random.default_rng(3)
    assert _check([_noisy_steps(rng, N, 3) for N in (LDS_CAP - 1, LDS_CAP, LDS_CAP + 1)], 2, 9, "N around the LDS cap") == 3


def test_kernel_longest_tail_of_the_default_window_domain():
    rng = np.random.default_rng(4)
    assert _check([_noisy_steps(rng, 16384, 3)], 2, 9, "16 384 samples") == 1


def test_kernel_ties_and_non_finite_samples():
    steps = np.repeat([1.0, 5.0, 2.0, 7.0], 10)
    cp, st = _device_cpts([np.zeros(40), steps], 3, 9)
    assert st.tolist() == [OK, OK] and cp.tolist() == [[0, 9, 18, 27, 40], [0, 10, 20, 30, 40]]
    rng = np.random.default_rng(5)
    ints = [rng.integers(-3, 4, 12).repeat(rng.integers(5, 12, 12)).astype(np.float64) for _ in range(6)]   # true ties
    consts = [np.full(77, 2.5), np.full(300, -1e6), np.zeros(2100)]
    assert _check(ints + consts, 5, 5, "integer steps and constants") == 9
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        s = _noisy_steps(rng, 150)
        s[rng.integers(0, 150)] = v
        bad.append(s)
    long_bad = _noisy_steps(rng, 2500)
    long_bad[2499] = np.nan
    assert _check(bad + [long_bad, _noisy_steps(rng, 150)], 5, 5, "NaN / infinity") == 1


def test_kernel_many_series_over_several_slices_of_the_scratch():
    """23 series of different lengths, both storage forms, walked by TWO workgroups: a dozen slices of the scratch buffer"""
    rng = np.random.default_rng(6)
    lens = [int(v) for v in rng.integers(40, 700, 20)] + [2300, 30, 2047]
    series = [_noisy_steps(rng, N) for N in lens]
    feasible = [N >= 7 * 7 for N in lens]
    assert sum(feasible) >= 18 and not all(feasible)
    assert _check(series, 6, 7, "two slots", max_slots=2) == sum(feasible)
    assert _check(series[:5], 6, 7, "one slot", max_slots=1, max_len=4096) == sum(feasible[:5])


def test_kernel_entry_refusals():
    import torch

    ctx, L = _lib.default_context(), _lib.load()
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    off = torch.tensor([0, 40], dtype=torch.int64, device="cuda")
    o = torch.zeros(8, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    assert L.wdx_selftest_optimal_cpts_dev(ctx.handle, p(d), p(off), 1, 3, 0, 40, 0, p(o), p(o), None) == _lib.WDX_ERR_UNSUPPORTED
    assert L.wdx_selftest_optimal_cpts_dev(ctx.handle, p(d), p(off), 1, MAX_BKPS + 1, 1, 40, 0, p(o), p(o), None) == _lib.WDX_ERR_INVALID
    assert L.wdx_selftest_optimal_cpts_dev(ctx.handle, p(d), p(off), 1, 3, 9, 16385, 0, p(o), p(o), None) == _lib.WDX_ERR_INVALID


# ---- whole reads --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mb():
    return oi.g14_minibatch()


def _check_fp(got, exp, what):
    for name in ("status", "fpt", "dwell", "stats", "refine_idx"):
        assert same(got[name], exp[name]), f"{what}: {name}"


@functools.lru_cache(maxsize=None)
def _boost_model(n_features=25):
    m = boost_ref.random_model(9, 3, 4, n_features, seed=83)
    trees = [(f, b, [False] * len(f), lv) for f, b, lv in m.trees]
    return models.Fpt_Boost(trees, m.n_features, m.scale, m.bias, {0: 7, 1: 1, 2: 10, 3: 4}, np.full(4, 0.3))


def test_g14_case_by_case_through_the_blocking_call():
    seen = set()
    for k, tag, row, a_s, a_e, seg, ref, exp in oi.g14_cases():
        fb = sig_proc.fingerprint_refine_batch(row.reshape(1, -1), [a_s], [a_e], sig_proc.SegParams(**seg),
                                               sig_proc.RefineParams(query=oi.g14()["consensus"], optimal_cpts=True, **ref))
        got = dict(status=fb.status[0], fpt=fb.fpt[0], dwell=fb.dwell[0], stats=fb.stats[0], refine_idx=fb.refine_idx[0])
        _check_fp(got, exp, f"case {k} ({tag})")
        seen.add(int(exp["status"]))
    assert seen == {0, 3, 6}
    assert not _lib.default_context().refine_optimal, "the option is put back after the call"


@pytest.mark.parametrize("path", ["as-is", "launch-chain", "exact-kernel"])
def test_g14_minibatch_blocking_call_whichever_kernel_segments_the_adapter(path):
    mb = _mb()
    ctx = _lib.default_context()
    opt = {"launch-chain": _lib.OPT_FAST_CHAIN_MIN_READS, "exact-kernel": _lib.OPT_EXACT_PATH}.get(path)
    L = _lib.load()
    try:
        if opt:
            ctx.set_option(opt, 1)
        _lib.check(L.wdx_kernel_time_reset(ctx.handle))
        _lib.check(L.wdx_kernel_timing(ctx.handle, 1))
        fb = sig_proc.fingerprint_refine_batch(mb["rows"], mb["a_s"], mb["a_e"], mb["params"], mb["refine"])
        ms, nl = C.c_double(0), C.c_int64(0)
        _lib.check(L.wdx_kernel_time(ctx.handle, _lib.K_REFINE_OPTIMAL, C.byref(ms), C.byref(nl)))
    finally:
        _lib.check(L.wdx_kernel_timing(ctx.handle, 0))
        if opt:
            ctx.set_option(opt, 0)
    _check_fp(vars(fb), mb, path)
    assert nl.value == 1 and ms.value > 0, "WDX_K_REFINE_OPTIMAL brackets the new kernel"


def test_window_beyond_the_exact_kernels_lds_and_a_tail_beyond_the_lds_cap():
    """a 12 000-sample adapter window (the exact kernel's big form segments it) whose barcode tail of ~2 800 scores takes
    the global-memory form of the dynamic programme, against the helper's composition"""
    mb = _mb()
    rng = np.random.default_rng(9)
    lv = np.concatenate([rng.normal(0, 1, 8), mb["consensus"], rng.normal(0, 1, 28)]) * 12.0 + 85.0
    dw = rng.integers(85, 116, lv.size)
    row = (np.repeat(lv, dw) + rng.normal(0, 1.5, int(dw.sum()))).astype(np.float32)
    assert 11264 < row.size <= 16384
    a_s, a_e = 100, row.size - 100
    fb = sig_proc.fingerprint_refine_batch(row.reshape(1, -1), [a_s], [a_e], mb["params"], mb["refine"])
    st, fpt, dwell, stats, idx = oc.refine_one(row, a_s, a_e, mb["seg"], mb["ref"], mb["consensus"], optimal=True)
    assert st == 0 and row.size - 36 - int(idx[2]) > LDS_CAP, (st, idx)
    _check_fp(dict(status=fb.status[0], fpt=fb.fpt[0], dwell=fb.dwell[0], stats=fb.stats[0], refine_idx=fb.refine_idx[0]),
              dict(status=st, fpt=fpt, dwell=dwell, stats=stats, refine_idx=idx), "big form")


def test_option_off_is_the_peak_branch():
    """the same reads without the field: what the oracle's peak branch gives, and not what the option gives"""
    mb = _mb()
    fb = sig_proc.fingerprint_refine_batch(mb["rows"], mb["a_s"], mb["a_e"], mb["params"], mb["refine_off"])
    o = orc.fingerprint_refine_batch(mb["rows"], mb["a_s"], mb["a_e"], orc.SegParams(**mb["seg"]),
                                     orc.RefineParams(query=mb["consensus"], **mb["ref"]))
    assert same(fb.status, o[4]) and same(fb.fpt, o[0]) and same(fb.dwell, o[1])
    rep = (o[4] == 0) | (o[4] == 6)
    assert same(fb.stats[rep], o[2][rep]) and same(fb.refine_idx[rep], o[3][rep]) and (o[4] == 0).sum() >= 5
    assert not same(fb.fpt, mb["fpt"])
    assert same(fb.stats[o[4] == 0], mb["stats"][o[4] == 0]), "everything up to the match is unchanged by the option"


def test_both_options_and_bad_parameters_are_refused():
    mb = _mb()
    ctx, L = _lib.Context(0), _lib.load()
    n, stride = mb["rows"].shape
    o = dict(fpt=np.empty((n, 25)), dwell=np.empty((n, 25), np.int64), stats=np.empty((n, 6)), idx=np.empty((n, 3), np.int32),
             status=np.empty(n, np.int32))

    def call(params):
        pc, rc = params.to_c(), mb["refine"].to_c()
        return L.wdx_fingerprint_refine_batch(ctx.handle, _lib.ptr(mb["rows"]), n, stride, _lib.ptr(mb["a_s"]), _lib.ptr(mb["a_e"]),
                                              None, C.byref(pc), C.byref(rc), _lib.ptr(o["fpt"]), _lib.ptr(o["dwell"]),
                                              _lib.ptr(o["stats"]), _lib.ptr(o["idx"]), _lib.ptr(o["status"]))
    try:
        assert L.wdx_ctx_set_option(ctx.handle, _lib.OPT_REFINE_OPTIMAL_CPTS, 2) == _lib.WDX_ERR_INVALID
        ctx.set_option(_lib.OPT_REFINE_OPTIMAL_CPTS, 1)
        ctx.set_option(_lib.OPT_LONG_REFINE_WINDOWS, 1)
        assert call(mb["params"]) == _lib.WDX_ERR_UNSUPPORTED
        ctx.set_option(_lib.OPT_LONG_REFINE_WINDOWS, 0)
        assert call(sig_proc.SegParams(**dict(mb["seg"], min_obs_per_base=0))) == _lib.WDX_ERR_UNSUPPORTED
        assert call(sig_proc.SegParams(**dict(mb["seg"], sig_norm="mean"))) == _lib.WDX_ERR_UNSUPPORTED
        assert call(mb["params"]) == 0, L.wdx_last_error()
        assert same(o["status"], mb["status"]) and same(o["fpt"], mb["fpt"])
    finally:
        ctx.close()
    with pytest.raises(ValueError, match="optimal_cpts and long_windows"):
        sig_proc.fingerprint_refine_batch(mb["rows"], mb["a_s"], mb["a_e"], mb["params"], mb["refine"], long_windows=True)


def test_g14_minibatch_device_resident_float32_and_int16_shard():
    import torch

    from warpdemux_amd.engine import AdcShard, DemuxEngine

    mb = _mb()
    n, stride = mb["rows"].shape
    d = lambda a: torch.from_numpy(np.array(a)).cuda()   # noqa: E731
    eng = DemuxEngine(np.zeros((2, 25)), 15, 0.1, mb["params"])
    try:
        def run(sig, **kw):
            fpt, dwell, stats, idx, status = eng.fingerprint_refine(sig, d(mb["a_s"]), d(mb["a_e"]), mb["refine"], max_len=stride, **kw)
            torch.cuda.synchronize()
            return dict(status=status.cpu().numpy(), fpt=fpt.cpu().numpy(), dwell=dwell.cpu().numpy(), stats=stats.cpu().numpy(),
                        refine_idx=idx.cpu().numpy())
        _check_fp(run(d(mb["rows"]), stride=stride), mb, "float32 rows")
        assert not eng.ctx.refine_optimal
        # an int16 shard stands for its calibrated rows: the same call on those is the yardstick
        adc, row_len, offset, scale = adc_inputs.quantise(mb["rows"], 7)
        cal = sig_proc.calibrate_adc(adc, row_len, offset, scale)
        want = run(d(cal), stride=stride)
        assert (want["status"] == mb["status"]).all()
        got = run(AdcShard(d(adc), d(row_len), d(offset), d(scale)))
        _check_fp(got, want, "int16 shard")
    finally:
        eng.close()


def test_g14_minibatch_pipeline_live_tick_and_boost_tail():
    import torch

    from warpdemux_amd.engine import DemuxEngine
    from warpdemux_amd.live import LiveDemux

    mb = _mb()
    n, stride = mb["rows"].shape
    pipe = pipeline.MinibatchPipeline(None, params=mb["params"], refine=mb["refine"])
    try:
        pipe.submit(0, mb["rows"], mb["a_s"], mb["a_e"], np.ones(n, np.uint8))
        r = pipe.wait(0)
    finally:
        pipe.close()
    _check_fp(vars(r.fingerprints), mb, "MinibatchPipeline(refine=...)")
    model = _boost_model()
    ld = LiveDemux(model=model, params=mb["params"], refine=mb["refine"], max_reads=16, max_samples=stride)
    try:
        rows = [np.ascontiguousarray(mb["rows"][i, : int(mb["a_e"][i]) + 100]) for i in range(n)]
        t = ld.tick(rows, mb["a_s"], mb["a_e"], want_fpt=True, want_dwell=True, want_stats=True, want_refine_idx=True)
    finally:
        ld.close()
    _check_fp(vars(t), mb, "LiveDemux tick")
    good = mb["status"] == 0
    assert (t.pred[good] >= -1).all() and np.isfinite(t.prob[good]).all() and np.isnan(t.prob[~good]).all()
    d = lambda a: torch.from_numpy(np.array(a)).cuda()   # noqa: E731
    eng = DemuxEngine(np.zeros((2, 25)), 15, 0.1, mb["params"])
    try:
        eng.set_boost(model)
        prob, pred, conf, status, idx, fpt, _ = eng.demux_boost(d(mb["rows"]), d(mb["a_s"]), d(mb["a_e"]), mb["refine"], stride=stride,
                                                               max_len=stride, want_fpt=True)
        torch.cuda.synchronize()
    finally:
        eng.close()
    assert same(status.cpu().numpy(), mb["status"]) and same(fpt.cpu().numpy(), mb["fpt"])
    rep = (mb["status"] == 0) | (mb["status"] == 6)
    assert same(idx.cpu().numpy()[rep], mb["refine_idx"][rep])
    assert same(prob.cpu().numpy(), t.prob) and same(pred.cpu().numpy().astype(t.pred.dtype), t.pred) and same(conf.cpu().numpy(), t.conf)


def test_g14_minibatch_through_a_feeder():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "feeder_optimal_check.py")], capture_output=True,
                       text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec and all(rec.values()), rec
