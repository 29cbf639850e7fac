"""The fingerprint kernels over the whole segmentation parameter domain the engine accepts (include/wdx.h,
wdx_seg_params): num_events 1 .. 253, barcode_num_events 1 .. 254, running_stat_width 0 .. 64, any min_obs_per_base,
adapter windows up to 16 384 samples.  The fast kernels take only part of it (num_events <= 126, reach <= 17, the
widths fast_combo knows); the rest -- suppression reach beyond 17 on the peak list and in position space, top-E
selection, event means and medians of 127 .. 254 segments, fingerprint_big_kernel beyond 11 200 samples -- runs on the
exact general kernel.  Every route into the kernels, bit for bit:

(a) g11 (tests/golden/make_golden_domain.py: the reference's own detect_results_to_fpt),
(b) the CPU oracle on styled batches at the same parameter points and a few random draws from the domain,
(c) the fused fingerprint -> DTW -> argmin host call with fingerprints of 127 .. 254 events,
(d) the call errors at the limits.

Needs a real MI355X: run with `pytest -m gpu`.
"""
import contextlib
import os
import zlib

import numpy as np
import pytest

from oracle import wdx_oracle as orc
from test_gpu_parity import _chain, _exact_path, _option, _params_from, _same, _styled_signal
from warpdemux_amd import _lib, sig_proc

pytestmark = pytest.mark.gpu

G11 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_param_domain.npz")
STYLES = ["gauss", "quantised", "integers", "heavy", "negative", "spiky", "flat_runs", "clipped_low"]
EDGES = [4095, 4096, 4097, 5119, 5120, 5121, 6143, 6144, 6145, 8191, 8192, 8193, 11199, 11200, 11201, 16383, 16384]
ROUTES = ("default", "chain", "exact_list", "exact_no_list", "packed_dev")


# ------------------------------------------------------------------------------------------ routes ----

@pytest.fixture(scope="module")
def eng():
    """one device engine (its own context) for the packed route; its reference set is swapped per K"""
    from warpdemux_amd.engine import DemuxEngine

    e = DemuxEngine(np.zeros((1, 25)), 15, 0.1, sig_proc.SegParams())
    yield e
    e.close()


def _host(route, mb, a_s, a_e, ph, ok):
    if route == "default":
        cm = contextlib.nullcontext()
    elif route == "chain":
        cm = _chain()
    else:
        cm = _option(_lib.OPT_EXACT_NO_PEAK_LIST, int(route == "exact_no_list"))
    with cm, (_exact_path() if route.startswith("exact") else contextlib.nullcontext()):
        fb = sig_proc.fingerprint_batch(mb, a_s, a_e, ph, success=ok)
    return fb.fpt, fb.dwell, fb.stats, fb.status


def _packed(eng, rows, a_s, a_e, ph, ok):
    """`DemuxEngine.fingerprint(..., offsets=...)` on the rows packed back to back (each row its own length)"""
    import torch

    K = ph.barcode_num_events
    if eng.K != K:
        eng.params = sig_proc.SegParams(barcode_num_events=K)
        eng.set_refs(np.zeros((1, K)), 15, 0.1)
    eng.params = ph
    lens = [r.size for r in rows]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ok_d = None if ok is None else d(np.asarray(ok, dtype=np.uint8))
    out = eng.fingerprint(d(np.concatenate(rows).astype(np.float32)), d(np.asarray(a_s, dtype=np.int32)),
                          d(np.asarray(a_e, dtype=np.int32)), offsets=d(off), max_len=max(lens), ok=ok_d)
    return tuple(t.cpu().numpy() for t in out)


def _run(route, eng, rows, a_s, a_e, ph, ok=None):
    if route == "packed_dev":
        return _packed(eng, rows, a_s, a_e, ph, ok)
    stride = max(r.size for r in rows)
    mb = np.full((len(rows), stride), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        mb[i, :r.size] = r
    return _host(route, mb, np.asarray(a_s, dtype=np.int32), np.asarray(a_e, dtype=np.int32), ph, ok)


def _check(got, ref, what):
    fpt, dwell, stats, status = got
    r_fpt, r_dwell, r_stats, r_status = ref
    assert np.array_equal(status, r_status), (what, np.flatnonzero(status != r_status), status[status != r_status],
                                              r_status[status != r_status])
    good = r_status == 0
    for name, a, b in (("fpt", fpt, r_fpt), ("dwell", dwell, r_dwell), ("stats", stats, r_stats)):
        bad = [i for i in np.flatnonzero(good) if not _same(a[i], b[i])]
        assert not bad, (what, name, bad)


# ------------------------------------------------------------------------------------- (a) g11 ----

def test_g11_reference_fixture_through_every_route(eng):
    """the reference's detect_results_to_fpt over the domain: statuses everywhere, fingerprints, dwell times and the six
    statistics bit for bit where it succeeded -- one read per call, through each route"""
    g = np.load(G11)
    n = int(g["n"])
    for route in ROUTES:
        for k in range(n):
            tag = str(g[f"tag_{k}"])
            a_start, a_end, ok = (int(v) for v in g[f"args_{k}"])
            ph, _ = _params_from(g, k)
            K = ph.barcode_num_events
            got = _run(route, eng, [g[f"row_{k}"]], [a_start], [a_end], ph, np.array([ok], dtype=np.uint8))
            ref = (g[f"fpt_{k}"].reshape(1, K), g[f"dwell_{k}"].reshape(1, K), g[f"stats_{k}"].reshape(1, 6),
                   np.array([int(g[f"status_{k}"])], dtype=np.int32))
            _check(got, ref, (route, k, tag))
            if route != "packed_dev" and ref[3][0] != 0:
                assert np.isnan(got[0]).all() and (got[1] == 0).all() and np.isnan(got[2]).all(), (route, k, tag)


# --------------------------------------------------------------------------------- (b) oracle sweep ----

def _points():
    """the distinct parameter settings of g11 (flagged when the reference succeeded on one of its reads) and six random
    draws from the whole domain"""
    inv = {0: "none", 1: "mean", 2: "median"}
    pts, first = [], {}
    g = np.load(G11)
    for k in range(int(g["n"])):
        pad, sig_norm, d, w, E, acc, seg_norm, K = (int(v) for v in g[f"params_{k}"])
        key = (sig_norm, d, w, E, acc, seg_norm, K)
        if key in first:
            pts[first[key]][1] |= int(g[f"status_{k}"]) == 0
            continue
        first[key] = len(pts)
        pts.append([str(g[f"tag_{k}"]), int(g[f"status_{k}"]) == 0,
                    dict(sig_norm=inv[sig_norm], min_obs_per_base=d, running_stat_width=w, num_events=E,
                         accept_less_cpts=bool(acc), seg_norm=inv[seg_norm], barcode_num_events=K)])
    pts = [pytest.param(kw, must_succeed, id=tag) for tag, must_succeed, kw in pts]
    rng = np.random.default_rng(20261016)
    for i in range(6):
        E = int(rng.integers(1, 254))
        kw = dict(sig_norm=str(rng.choice(["none", "none", "mean", "median"])),
                  min_obs_per_base=int(rng.choice([0, 1, 2, 5, 9, 17, 18, 23, 40, 90, 300, 1000])),
                  running_stat_width=int(rng.integers(0, 65)), num_events=E, accept_less_cpts=bool(rng.integers(0, 2)),
                  seg_norm=str(rng.choice(["mean", "median", "none"])),
                  barcode_num_events=int(min(254, rng.integers(1, E + 3))))
        pts.append(pytest.param(kw, False, id=f"random{i}"))
    return pts


def _window_lengths(rng, E, n):
    """full window lengths (padding included): the shrink regime with n/E and n/2E on .5 ties, every capacity edge,
    and spread lengths"""
    out = []
    for i in range(n):
        c = i % 4
        if c == 0:    # parameter shrink: a few samples per event
            x = rng.uniform(2.0, 40.0)
            ln = int(E * x)
            if i % 8 == 0:
                m = 2 * int(rng.integers(1, 20)) + 1        # n / 2E = m / 2 (tie)
                ln = E * m
            elif i % 8 == 4 and E % 2 == 0:
                ln = (E // 2) * (2 * int(rng.integers(2, 30)) + 1)   # n / E on a tie
        elif c == 1:
            ln = EDGES[(i // 4) % len(EDGES)]
        else:
            ln = int(rng.integers(1500, 16385)) if c == 2 else int(rng.integers(2500, 9000))
        out.append(int(min(max(ln, 3), 16384)))
    return out


def _sweep_batch(seed, E, n):
    rng = np.random.default_rng(seed)
    pad = int(rng.choice([0, 30, 100]))
    rows, a_s, a_e = [], [], []
    for i, nw in enumerate(_window_lengths(rng, E, n)):
        st = 0 if i % 10 == 3 else int(rng.integers(0, 40)) + pad     # i % 10 == 3: padding clipped at the row start
        body = max(nw - 2 * pad, 1)
        ln = st + body + pad + int(rng.integers(0, 60))
        rows.append(_styled_signal(rng, ln, STYLES[i % len(STYLES)]))
        a_s.append(st)
        a_e.append(st + body)
    ok = (rng.uniform(size=n) > 0.05).astype(np.uint8)
    return rows, np.array(a_s, dtype=np.int32), np.array(a_e, dtype=np.int32), ok, pad


@pytest.mark.parametrize("kw,must_succeed", _points())
def test_parameter_domain_sweep_vs_oracle(kw, must_succeed, eng, request):
    """96 styled reads per parameter point (quantised and integer-valued rows too: the oracle defines the tie rule),
    windows across the shrink regime, every capacity edge, 11 200 / 11 201 and 16 384 samples; a few with ok = 0"""
    rows, a_s, a_e, ok, pad = _sweep_batch(zlib.crc32(request.node.callspec.id.encode()), kw["num_events"], 96)
    kw = dict(kw, padding=pad, outlier_thresh=5.0)
    ph, po = sig_proc.SegParams(**kw), orc.SegParams(**kw)
    stride = max(r.size for r in rows)
    mb = np.full((len(rows), stride), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        mb[i, :r.size] = r
    ref = orc.fingerprint_batch(mb, a_s, a_e, po, ok=ok)
    # where the reference succeeded at this setting, so must some reads here, or the comparison pinned no fingerprint
    assert not must_succeed or (ref[3] == 0).sum() >= 8, int((ref[3] == 0).sum())
    for route in ROUTES:
        _check(_run(route, eng, rows, a_s, a_e, ph, ok), ref, (route, kw))


# ---------------------------------------------------------------------- (c) fused path, long fingerprints ----

@pytest.mark.parametrize("E,d,w,K,window", [(126, 6, 12, 127, 15), (200, 20, 40, 201, None), (253, 6, 12, 254, 40)])
def test_demux_batch_with_long_fingerprints_vs_oracle(E, d, w, K, window):
    """sig_proc.demux_batch (fingerprint -> DTW against resident references -> argmin, one host call) with fingerprints
    of K = 127 / 201 / 254 events: the oracle's fingerprints -> dtw_matrix -> argmin_rows, float32 distances bit for
    bit (DTW series beyond L = 200)"""
    kw = dict(num_events=E, min_obs_per_base=d, running_stat_width=w, barcode_num_events=K)
    rows, a_s, a_e, ok, pad = _sweep_batch(K, E, 128)
    kw["padding"] = pad
    stride = max(r.size for r in rows)
    mb = np.full((len(rows), stride), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        mb[i, :r.size] = r
    fpt, dwell, stats, status = orc.fingerprint_batch(mb, a_s, a_e, orc.SegParams(**kw), ok=ok)
    good = status == 0
    assert good.sum() >= 64
    rng = np.random.default_rng(K)
    refs = fpt[good][:9] + rng.normal(0, 0.05, (9, K))
    sig_proc.set_references(refs, window, 0.1)
    res = sig_proc.demux_batch(mb, a_s, a_e, sig_proc.SegParams(**kw), success=ok, want_dist=True, want_fpt=True)
    assert np.array_equal(res.status, status)
    assert _same(res.fpt[good], fpt[good])
    D = orc.dtw_matrix(fpt[good], refs, window, 0.1)
    assert res.dist.dtype == np.float32
    assert np.array_equal(res.dist[good].view(np.uint32), D.view(np.uint32)), np.count_nonzero(res.dist[good] != D)
    assert np.array_equal(res.call[good], orc.argmin_rows(D))
    assert (res.call[~good] == -1).all() and np.isnan(res.dist[~good]).all()


# ------------------------------------------------------------------------------- (d) refusals at the limits ----

def _one_read(**kw):
    rng = np.random.default_rng(3)
    row = _styled_signal(rng, 3000, "gauss")
    return sig_proc.fingerprint_batch(row.reshape(1, -1), [100], [2900], sig_proc.SegParams(**kw))


@pytest.mark.parametrize("kw,exc,msg", [
    (dict(num_events=254, barcode_num_events=25), NotImplementedError, r"num_events must be in \[1, 253\]"),
    (dict(running_stat_width=65), NotImplementedError, r"running_stat_width must be in \[0, 64\]"),
    (dict(num_events=253, barcode_num_events=255), ValueError, r"barcode_num_events must be in \[1, 254\]"),
    (dict(num_events=0), ValueError, r"num_events must be in \[1, 253\]"),
    (dict(padding=-1), ValueError, r"padding must be >= 0"),
])
def test_limits_are_call_errors(kw, exc, msg):
    with pytest.raises(exc, match=msg):
        _one_read(**kw)


def test_d0_and_w0_are_per_read_statuses():
    """min_obs_per_base = 0 (scipy's find_peaks refuses distance 0: "unknown") and running_stat_width = 0 (no scores:
    "event segmentation failed") are not call errors: each read gets the oracle's status; the limits themselves run"""
    for kw in (dict(min_obs_per_base=0), dict(running_stat_width=0), dict(num_events=253, barcode_num_events=254),
               dict(running_stat_width=64), dict(num_events=1, barcode_num_events=1)):
        fb = _one_read(**kw)
        rng = np.random.default_rng(3)
        row = _styled_signal(rng, 3000, "gauss")
        fpt, dwell, stats, status = orc.fingerprint_batch(row.reshape(1, -1), np.array([100], dtype=np.int32),
                                                          np.array([2900], dtype=np.int32), orc.SegParams(**kw))
        assert np.array_equal(fb.status, status), kw
        assert _same(fb.fpt, fpt) and _same(fb.dwell, dwell) and _same(fb.stats, stats), kw
    assert _one_read(min_obs_per_base=0).status[0] == 5 and _one_read(running_stat_width=0).status[0] == 3
