"""The wide-window DTW kernel (WDX_OPT_WIDE_DTW = 24: effective windows 33 .. L at L <= 256) by name, against the oracle.

Every case first asks the library which kernel it ran (wdx_dtw_last_launch: family "wide") and then compares float32 distances
bit for bit with oracle.wdx_oracle.dtw_matrix and the argmin with orc.argmin_rows (test_gpu_parity._check_dist; no tolerance).
Where the case is too large for the oracle pair by pair, the oracle checks a fixed row subset and EVERY row is compared with
the default route (option off: the scratch rows), which tests/test_gpu_dtw_dispatch.py pins to the oracle.  Without the
option every case here fails at ``set_option(24, ...)``.

Shapes are the smallest at which each edge exists: strips are 32 columns wide, so windows and lengths sit on both sides of
32 / 64 / 96; 65 reads are a full and a partial wave; 8 192 reads are where the row-major layout starts."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import refine_inputs as ri, wide_inputs as wi
from helpers.dtw_cases import (RL, RM, TM, effective_window, equal_infinities, fused_rule, kernel_of, last_route, nonfinite_reads,
                               nonfinite_refs, options, oracle_dtw, subset_rows)
from oracle import wdx_oracle as orc
from test_gpu_parity import _check_dist, _same
from warpdemux_amd import _lib, live, parallel_distances as pdist, pipeline, sig_proc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PENALTIES = (None, 0.0, 0.1, 1.5)
WIDE = ("wide", 0, False)


@contextlib.contextmanager
def wide(ctx=None):
    """WDX_OPT_WIDE_DTW = 1 on the context for the duration of the block"""
    ctx = ctx or _lib.default_context()
    ctx.set_option(_lib.OPT_WIDE_DTW, 1)
    try:
        yield ctx
    finally:
        ctx.set_option(_lib.OPT_WIDE_DTW, 0)


def _check(X, Y, w, p, layout, fused=None):
    """nearest_reference on the wide kernel in `layout` against the oracle; returns (route, distances, argmin)"""
    got, am = pdist.nearest_reference(X, Y, w, p)
    r = last_route()
    assert kernel_of(r) == WIDE + (layout,), r
    assert r.launches == 1 and r.window == effective_window(w, X.shape[1]), r
    assert r.grid_x == ((Y.shape[0] if layout == RL else X.shape[0]) + 63) // 64, r
    if fused is not None:
        assert r.fused == fused, r
    ref = oracle_dtw(X, Y, w, p)
    _check_dist(got, ref)
    assert np.array_equal(am, orc.argmin_rows(ref))
    return r, got, am


def _default_route(X, Y, w, p, family="scratch"):
    """the same call with the option off: the parent commit's kernel"""
    ctx = _lib.default_context()
    assert not ctx.wide_dtw
    D, am = pdist.nearest_reference(X, Y, w, p)
    assert last_route().family == family, last_route()
    return D, am


# ------------------------------------------------------------------------------------ 1. every window ----

WINDOWS = {
    33: [33, None, 0, 36],
    34: [33, 34, None, 0, 37],
    70: list(range(33, 71)) + [None, 0, 73],
    110: [33, 47, 48, 49, 63, 64, 65, 96, 97, 109, 110, None],     # both sides of every strip edge
    256: [33, 128, 255, None],
}


@pytest.mark.parametrize("L", sorted(WINDOWS))
def test_every_window_read_minor(L):
    """65 reads x 3 references (a full and a partial wave), four penalties"""
    rng = np.random.default_rng(2400 + L)
    X, Y = rng.normal(size=(65, L)), rng.normal(size=(3, L))
    with wide():
        for w in WINDOWS[L]:
            for p in PENALTIES:
                r, _, _ = _check(X, Y, w, p, TM, fused=False)
                assert r.window == (L if (w is None or w <= 0 or w > L) else w) and r.window >= 33


def test_option_values_and_the_shapes_it_leaves_alone():
    """2 is refused; L = 257 stays on the scratch rows and window 32 on band<32> with the option on; off, nothing moved"""
    ctx = _lib.default_context()
    rng = np.random.default_rng(2401)
    for bad in (2, -1, 256):
        with pytest.raises(ValueError, match="WDX_OPT_WIDE_DTW"):
            ctx.set_option(_lib.OPT_WIDE_DTW, bad)
    assert not ctx.wide_dtw
    X, Y = rng.normal(size=(65, 257)), rng.normal(size=(2, 257))
    X2, Y2 = rng.normal(size=(65, 110)), rng.normal(size=(3, 110))
    with wide():
        got, am = pdist.nearest_reference(X, Y, None, 0.1)
        assert kernel_of(last_route()) == ("scratch", 0, False, TM)
        ref = oracle_dtw(X, Y, None, 0.1)
        _check_dist(got, ref)
        assert np.array_equal(am, orc.argmin_rows(ref))
        pdist.nearest_reference(X2, Y2, 32, 0.1)
        assert kernel_of(last_route()) == ("band", 32, False, TM)
        pdist.nearest_reference(X2, Y2, 33, 0.1)
        assert last_route().family == "wide"
    pdist.nearest_reference(X2, Y2, 33, 0.1)
    assert last_route().family == "scratch"
    # for one call of the non-reference-named function
    pdist.nearest_reference(X2, Y2, None, 0.1, wide_dtw=True)
    assert last_route().family == "wide" and not ctx.wide_dtw


# ------------------------------------------------------------------------- 2. layouts and lane edges ----

@pytest.mark.parametrize("L,w", [(40, 33), (110, None)])
@pytest.mark.parametrize("nX", [1, 63, 64, 65, 8191])
def test_read_minor_lane_edges(nX, L, w):
    rng = np.random.default_rng(2500 + nX + L)
    X, Y = rng.normal(size=(nX, L)), rng.normal(size=(1 if nX < 64 else 2, L))     # (1 read x 1 reference: lanes stay the reads)
    with wide():
        _check(X, Y, w, 0.1, TM)


@pytest.mark.parametrize("L,w", [(40, 33), (110, None), (70, 50)])
@pytest.mark.parametrize("nX", [8192, 8193, 8255])
def test_row_major_lane_edges_and_every_row_against_the_default_route(nX, L, w):
    """a lane reads its own row; the inactive lanes of the last wave are clamped to row nA - 1"""
    rng = np.random.default_rng(2600 + nX + L)
    X, Y = rng.normal(size=(nX, L)), rng.normal(size=(2, L))
    with wide():
        got, am = pdist.nearest_reference(X, Y, w, 0.1)
        r = last_route()
    assert kernel_of(r) == WIDE + (RM,) and r.launches == 1 and r.grid_x == (nX + 63) // 64, r
    rows = subset_rows(nX, drawn=600, seed=nX)
    ref = oracle_dtw(X[rows], Y, w, 0.1)
    _check_dist(got[rows], ref)
    assert np.array_equal(am[rows], orc.argmin_rows(ref))
    D0, am0 = _default_route(X, Y, w, 0.1)
    assert _same(D0, got) and np.array_equal(am0, am)


@pytest.mark.parametrize("L,w", [(40, 33), (110, None)])
@pytest.mark.parametrize("nX,nY", [(1, 66), (63, 65)])
def test_refs_as_lanes(nX, nY, L, w):
    """few reads, more references: the lanes run over the resident transposed references; a duplicated reference ties"""
    rng = np.random.default_rng(2700 + nX + L)
    X, Y = rng.normal(size=(nX, L)), rng.normal(size=(nY, L))
    Y[nY - 1] = Y[0]
    X[0] = Y[0] + 1e-3
    with wide():
        _, _, am = _check(X, Y, w, 0.1, RL, fused=False)
    assert am[0] == 0


# ------------------------------------------------------------------------------- 3. non-finite data ----

@pytest.mark.parametrize("L,w", [(40, 33), (110, None)])
def test_nonfinite_reads_and_references(L, w):
    """NaN / inf samples in reads and references, a whole wave of NaN rows and a wave with exactly one, through the
    read-minor form (flags from the transpose) and on row-major device rows (the kernel's lazy sweep); the six-operation,
    product and settle-everything modes of WDX_OPT_DTW_UNFUSED give the same bits"""
    import torch

    from warpdemux_amd.engine import DemuxEngine

    rng = np.random.default_rng(2800 + L)
    X, Y = nonfinite_reads(rng, 200, L), nonfinite_refs(rng, L)
    ref = oracle_dtw(X, Y, w, 0.1)
    assert np.isnan(ref[64:128]).all() and np.isnan(ref[145]).all() and np.isfinite(ref[130, :4]).all()
    with wide():
        for mode in (0, 1, 2):
            with options(unfused=mode):
                got, am = pdist.nearest_reference(X, Y, w, 0.1)
            assert kernel_of(last_route()) == WIDE + (TM,)
            _check_dist(got, ref)
            assert np.array_equal(am, orc.argmin_rows(ref))
    Xl = nonfinite_reads(rng, 8200, L)
    refl = oracle_dtw(Xl, Y, w, 0.1)
    eng = DemuxEngine(Y, w, 0.1, sig_proc.SegParams(barcode_num_events=L), wide_dtw=True)
    try:
        Xd = torch.from_numpy(Xl).to(eng.tdev)
        for mode in (0, 1, 2):
            with options(eng.ctx, unfused=mode):
                d, am = eng.dtw(Xd, want_argmin=True)
                eng.ctx.synchronize()
            assert kernel_of(last_route(eng.ctx)) == WIDE + (RM,)
            _check_dist(d.cpu().numpy(), refl)
            assert np.array_equal(am.cpu().numpy(), orc.argmin_rows(refl))
    finally:
        eng.close()


@pytest.mark.parametrize("L,w", [(40, 33), (110, None)])
def test_equal_infinities_are_settled_behind_the_kernel(L, w):
    """the same infinity at one index of a read and a reference: NaN on the diagonal (dtw_settle_inf runs behind the wide
    kernel as behind every other), +inf off it; the three modes of WDX_OPT_DTW_UNFUSED give the same bits"""
    rng = np.random.default_rng(2900 + L)
    X, Y = equal_infinities(rng, 70, L)
    with wide():
        for mode in (0, 1, 2):
            with options(unfused=mode):
                _, got, _ = _check(X, Y, w, 0.1, TM)
            assert np.isnan(got[2, 2]) and np.isinf(got[7, 7])


# --------------------------------------------------------------------------- 4. grid split and argmin ----

@pytest.mark.parametrize("nY", [1, 16, 17, 33, 100, 851])
def test_reference_split_over_grid_y_and_the_argmin(nY):
    """130 reads: one block walks `rpb` references, the argmin is the separate kernel unless nY = 1; exact ties in different
    reference blocks go to the lowest index; a NaN reference wins every row"""
    L, w = 40, 33
    rng = np.random.default_rng(3000 + nY)
    X, Y = rng.normal(size=(130, L)), rng.normal(size=(nY, L))
    if nY >= 17:
        Y[nY - 1] = Y[2]          # a tie between the first and the last reference block
        Y[16] = Y[2]              # ... and the second
        X[5] = Y[2]               # distance 0 to all three
    with wide():
        r, _, am = _check(X, Y, w, 0.1, TM, fused=nY == 1)
        assert r.fused == fused_rule(130, nY)
        assert r.grid_y == (nY + r.rpb - 1) // r.rpb and (nY == 1 or r.grid_y > 1), r
        if nY >= 17:
            assert am[5] == 2
        k = nY // 2
        Y[k, L // 2] = np.nan
        _, got, am = _check(X, Y, w, 0.1, TM, fused=nY == 1)
        assert (am == k).all() and np.isnan(got[:, k]).all()


def test_one_large_row_major_launch_with_the_fused_argmin():
    """131 073 reads x 3 references at L = 34 / w = 33: ONE launch of 2 049 blocks (the scratch rows take three), the argmin
    folded into it; the oracle on a row subset, every row against the default route"""
    nX, L, w = 131_073, 34, 33
    rng = np.random.default_rng(3100)
    X, Y = rng.normal(size=(nX, L)), rng.normal(size=(3, L))
    X[nX - 1, 3] = np.nan
    with wide():
        got, am = pdist.nearest_reference(X, Y, w, 0.1)
        r = last_route()
    assert kernel_of(r) == WIDE + (RM,) and r.launches == 1 and r.grid_x == 2049 and r.grid_y == 1, r
    assert fused_rule(nX, 3) and r.fused and r.rpb == 3
    rows = subset_rows(nX, boundaries=(65536, 131072), seed=31)
    ref = oracle_dtw(X[rows], Y, w, 0.1)
    _check_dist(got[rows], ref)
    assert np.array_equal(am[rows], orc.argmin_rows(ref)) and np.isnan(got[nX - 1]).all()
    D0, am0 = _default_route(X, Y, w, 0.1)
    assert last_route().launches == 3
    assert _same(D0, got) and np.array_equal(am0, am)


# --------------------------------------------------------------------------------- 5. fused entries ----

def _d(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _fused_engine(K, window, on=True):
    """an engine whose 10 references are fingerprints of the batch's own reads"""
    from warpdemux_amd.engine import DemuxEngine

    b = wi.synth_batch()
    p = sig_proc.SegParams(barcode_num_events=K, padding=b["padding"])
    fb = sig_proc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], p, success=b["ok"])
    refs = np.ascontiguousarray(fb.fpt[fb.status == 0][:10]) + 0.01
    assert refs.shape == (10, K)
    return DemuxEngine(refs, window, 0.1, p, wide_dtw=True) if on else DemuxEngine(refs, window, 0.1, p), refs


def _check_fused(res, fpt_alone, status_alone, refs, window, start, min_good=0.5):
    """dist / call / counts of a fused entry against the oracle on the entry's own fingerprints"""
    status, fpt, dist, call, counts = (t.cpu().numpy() for t in (res.status, res.fpt, res.dist, res.call, res.counts))
    assert _same(fpt, fpt_alone.cpu().numpy()) and _same(status, status_alone.cpu().numpy())
    good = status == 0
    assert good.sum() >= min_good * len(status) and (~good).sum() >= 3
    nY = refs.shape[0]
    ref = oracle_dtw(fpt[good], refs, window, 0.1)
    _check_dist(np.ascontiguousarray(dist[good]), ref)
    assert np.isnan(dist[~good]).all() and np.isnan(fpt[~good]).all()
    assert np.array_equal(call[good], orc.argmin_rows(ref)) and (call[~good] == -1).all()
    assert np.array_equal(counts, start + np.bincount(np.where(call < 0, nY, call), minlength=nY + 1))
    assert counts[nY] - start[nY] == (~good).sum()
    return status, fpt, dist, call, counts


@pytest.mark.parametrize("n", [300, 8200], ids=["transposed-branch", "row-major-branch"])
@pytest.mark.parametrize("K,window", [(110, None), (40, 33)])
def test_demux_on_synthetic_reads_and_an_int16_shard(K, window, n):
    import torch

    from warpdemux_amd.engine import AdcShard

    eng, refs = _fused_engine(K, window)
    b = wi.tiled(wi.synth_batch(), n)
    stride = b["rows"].shape[1]
    rows, a_s, a_e, ok = _d(b["rows"]), _d(b["a_s"]), _d(b["a_e"]), _d(b["ok"])
    start = np.arange(eng.nY + 1, dtype=np.int64) * 7
    res = eng.demux(rows, a_s, a_e, ok=ok, counts=_d(start), want_fpt=True, stride=stride, max_len=stride)
    torch.cuda.synchronize()
    r = last_route(eng.ctx)
    assert kernel_of(r) == WIDE + (RM if n >= 8192 else TM,) and r.launches == 1 and r.fused == fused_rule(n, eng.nY), r
    fpt, _, _, status = eng.fingerprint(rows, a_s, a_e, ok=ok, stride=stride, max_len=stride)
    want = _check_fused(res, fpt, status, refs, window, start)
    # the int16 shard of the same rows: wdx_demux_adc_dev
    shard = AdcShard(_d(b["adc"]), _d(b["row_len"]), _d(b["offset"]), _d(b["scale"]))
    res16 = eng.demux(shard, a_s, a_e, ok=ok, counts=_d(start), want_fpt=True, max_len=stride)
    torch.cuda.synchronize()
    assert last_route(eng.ctx).family == "wide"
    got = tuple(t.cpu().numpy() for t in (res16.status, res16.fpt, res16.dist, res16.call, res16.counts))
    for g, w_ in zip(got, want):
        assert _same(g, w_)


def test_demux_without_the_keyword_is_refused_as_before():
    eng, _ = _fused_engine(40, 33, on=False)
    b = wi.synth_batch()
    stride = b["rows"].shape[1]
    with pytest.raises(NotImplementedError, match="window <= 32"):
        eng.demux(_d(b["rows"]), _d(b["a_s"]), _d(b["a_e"]), ok=_d(b["ok"]), stride=stride, max_len=stride)
    # beyond the wide kernel's length the refusal stays with the option on
    from warpdemux_amd.engine import DemuxEngine

    long_ = DemuxEngine(np.zeros((2, 257)), None, 0.1, sig_proc.SegParams(barcode_num_events=257), wide_dtw=True)
    try:
        with pytest.raises(NotImplementedError, match="window <= 32"):
            long_.demux(_d(b["rows"]), _d(b["a_s"]), _d(b["a_e"]), ok=_d(b["ok"]), stride=stride, max_len=stride)
    finally:
        long_.close()


@pytest.mark.parametrize("n", [96, 8200], ids=["transposed-branch", "row-major-branch"])
def test_demux_refine_and_its_int16_shard(n):
    """wdx_demux_refine_dev / _adc_dev on tRNA-like reads with 40 refined events, unbanded references"""
    import torch

    from warpdemux_amd.engine import AdcShard, DemuxEngine

    K = wi.REFINE_K
    b = wi.tiled(wi.refine_batch(), n)
    stride = b["rows"].shape[1]
    hr = sig_proc.RefineParams(query=ri.consensus(), **wi.REFINE_REF)
    p = sig_proc.SegParams(barcode_num_events=K, **wi.REFINE_SEG)
    refs = np.random.default_rng(3300).normal(size=(6, K))
    eng = DemuxEngine(refs, None, 0.1, p, wide_dtw=True)
    try:
        rows, a_s, a_e, ok = _d(b["rows"]), _d(b["a_s"]), _d(b["a_e"]), _d(b["ok"])
        start = np.full(eng.nY + 1, 3, dtype=np.int64)
        res, dwell, stats, idx = eng.demux_refine(rows, a_s, a_e, hr, ok=ok, counts=_d(start), stride=stride, max_len=stride)
        torch.cuda.synchronize()
        r = last_route(eng.ctx)
        assert kernel_of(r) == WIDE + (RM if n >= 8192 else TM,) and r.window == K, r
        fr = eng.fingerprint_refine(rows, a_s, a_e, hr, ok=ok, stride=stride, max_len=stride)
        want = _check_fused(res, fr[0], fr[4], refs, None, start, min_good=0.3)     # (every sixth read has no consensus)
        st = want[0]
        assert st[ri.I_DEAD] == 1 and st[ri.I_SHORT] == 3 and (st == 6).sum() >= 3
        shard = AdcShard(_d(b["adc"]), _d(b["row_len"]), _d(b["offset"]), _d(b["scale"]))
        res16, dwell16, stats16, idx16 = eng.demux_refine(shard, a_s, a_e, hr, ok=ok, counts=_d(start), max_len=stride)
        torch.cuda.synchronize()
        assert last_route(eng.ctx).family == "wide"
        got = tuple(t.cpu().numpy() for t in (res16.status, res16.fpt, res16.dist, res16.call, res16.counts))
        for g, w_ in zip(got, want):
            assert _same(g, w_)
        assert _same(dwell16.cpu().numpy(), dwell.cpu().numpy()) and _same(idx16.cpu().numpy(), idx.cpu().numpy())
    finally:
        eng.close()


# ---------------------------------------------------------------------- 6. host ways in and the tails ----

@functools.lru_cache(maxsize=None)
def _blocking_default():
    """the 64-read minibatch through the blocking call with the option off: the scratch rows"""
    b = wi.synth_batch()
    p = sig_proc.SegParams(barcode_num_events=110, padding=b["padding"])
    refs = wi.host_refs()
    sig_proc.set_references(refs, None, 0.1)
    db = sig_proc.demux_batch(b["rows"][:64], b["a_s"][:64], b["a_e"][:64], p, success=b["ok"][:64], want_fpt=True)
    assert last_route().family == "scratch"
    good = db.status == 0
    assert good.sum() >= 40 and (~good).sum() >= 2
    _check_dist(np.ascontiguousarray(db.dist[good]), oracle_dtw(db.fpt[good], refs, None, 0.1))
    return b, p, refs, db


def _assert_like_blocking(r, db, what):
    assert _same(r.status, db.status) and _same(r.call, db.call) and _same(r.dist, db.dist), what
    if getattr(r, "fpt", None) is not None:
        assert _same(r.fpt, db.fpt), what


def test_minibatch_pipeline():
    b, p, refs, db = _blocking_default()
    pl = pipeline.MinibatchPipeline(refs, None, 0.1, p, wide_dtw=True)
    try:
        pl.submit(0, b["rows"][:64], b["a_s"][:64], b["a_e"][:64], success=b["ok"][:64], want_fpt=True)
        assert last_route(pl.ctx).family == "wide"          # (a pipelined minibatch reports at its submit)
        pl.submit_adc(1, b["adc"][:64], b["row_len"][:64], b["offset"][:64], b["scale"][:64], b["a_s"][:64], b["a_e"][:64],
                      success=b["ok"][:64], want_fpt=True)
        r0, r1 = pl.wait(0), pl.wait(1)
    finally:
        pl.ctx.close()
    _assert_like_blocking(r0, db, "submit")
    _assert_like_blocking(r1, db, "submit_adc")


def test_live_tick():
    b, p, refs, db = _blocking_default()
    ld = live.LiveDemux(refs, None, 0.1, p, max_reads=64, max_samples=9000, wide_dtw=True)
    try:
        stride = b["rows"].shape[1]
        rows = [np.ascontiguousarray(b["rows"][i, : min(int(b["row_len"][i]) + 200, stride)]) for i in range(64)]
        t = ld.tick(rows, b["a_s"][:64], b["a_e"][:64], success=b["ok"][:64], want_fpt=True)
        assert last_route(ld.ctx).family == "wide"
    finally:
        ld.close()
    _assert_like_blocking(t, db, "LiveDemux.tick")


def test_feeder_round(tmp_path):
    """the serving context lives in the feeder's own process: the helper has it report its option and its last route when
    `_serve` closes it"""
    import json

    out = str(tmp_path / "feeder.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "feeder_wide_check.py"), out],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = np.load(out)
    _b, _p, _refs, db = _blocking_default()
    assert _same(got["status"], db.status) and _same(got["call"], db.call) and _same(got["dist"], db.dist)
    with open(out + ".route.json") as fh:
        served = json.load(fh)
    assert served["wide_dtw"] is True and served["family"] == "wide" and served["layout"] == TM, served
    assert served["window"] == 110 and served["launches"] == 1, served


def _svm_model(k=4, n_train=60, L=40, seed=3):
    from sklearn.svm import SVC

    from warpdemux_amd.models import DTW_SVM

    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(k, L))
    y = np.arange(n_train) % k
    Xtr = centers[y] + 0.6 * rng.normal(size=(n_train, L))
    Ktr = np.exp(-0.05 * orc.dtw_matrix(Xtr, Xtr, None, 0.1).astype(np.float64))
    svc = SVC(kernel="precomputed", probability=True, random_state=0).fit(Ktr, y)
    sp = orc.svm_params(svc)
    model = DTW_SVM(Xtr, *sp[:6], {i: i + 1 for i in range(k)}, np.full(k, 0.2), None, 0.1, gamma=0.05, block_size=500)
    return model, centers


def test_classifier_tails_give_the_same_bits_on_both_routes():
    """a sklearn-fitted DTW_SVM and a DTW_MLP with window=None at L = 40 (wdx_dtw_svm_predict / wdx_dtw_mlp_predict: the
    DTW in front of the tail goes through the same dispatcher)"""
    pytest.importorskip("sklearn")
    from helpers import mlp_ref
    from warpdemux_amd import models

    svm, centers = _svm_model()
    rng = np.random.default_rng(3500)
    X = centers[rng.integers(0, 4, 150)] + 0.6 * rng.normal(size=(150, 40))
    est = mlp_ref.random_mlp(svm._X.shape[0], (16,), 5, np.float32, "relu", seed=9)
    mlp = models.from_reference(mlp_ref.DTW_MLP(est, svm._X, {i: 3 * i + 1 for i in range(5)}, np.linspace(0.05, 0.3, 5),
                                                window=None, penalty=0.1))
    for model in (svm, mlp):
        off = model.predict(X, nproc=1)
        assert last_route().family == "scratch"
        with wide():
            on = model.predict(X, nproc=1)
            assert last_route().family == "wide"
        assert len(on) == len(off) >= 2
        for a, c in zip(on, off):
            assert _same(np.asarray(a), np.asarray(c))
        assert np.unique(np.asarray(off[1]), axis=0).shape[0] >= 100     # (the probabilities follow the distances)
    assert len(set(np.asarray(svm.predict(X, nproc=1)[0]).tolist())) >= 2     # (the fitted model separates its classes)
