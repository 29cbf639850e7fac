"""Inputs of the long-window refinement tests (tests/test_gpu_long_refine.py, tests/test_oracle_refine_long.py,
tests/helpers/feeder_refine_long_check.py): tRNA-like reads -- random leader | the consensus shape | 30 barcode events, as
tests/helpers/refine_inputs.py builds them, with the dwell times scaled up -- whose adapter windows lie around
WDX_MAX_ADAPTER_SAMPLES = 16 384 and up to (and beyond) WDX_MAX_LONG_ADAPTER_SAMPLES = 65 536 samples, which
``long_windows=True`` (WDX_OPT_LONG_REFINE_WINDOWS) serves on the consensus-refinement branch.

Every batch is held against the CPU oracle, which has no window limit, where it is built: the kinds of reads it was built
to hold do occur before anything runs on a GPU."""
import functools
import os

import numpy as np

from helpers import adc_inputs
from helpers.refine_inputs import PADDING, REF, SEG, consensus
from oracle import wdx_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
CAP, LONG_CAP = 16384, 65536
K = 25
INV = {0: "none", 1: "mean", 2: "median"}


def g13():
    return np.load(os.path.join(GOLDEN, "g13_refine_long.npz"), allow_pickle=False)


def params_from(g, k):
    """(segmentation keywords, refinement keywords, clip bounds in float64) of record k: g8's layout plus clip64_k"""
    pad, d, w, E, seg_norm, e2, keep, sub_norm, p0, p1, p2, p3, ub_s, lb_e, ub_e = (int(v) for v in g[f"seg_{k}"])
    thr, pen = (float(v) for v in g[f"fl_{k}"])
    seg = dict(padding=pad, min_obs_per_base=d, running_stat_width=w, num_events=E, seg_norm=INV[seg_norm],
               outlier_thresh=thr, barcode_num_events=keep)
    ref = dict(subseq_norm=INV[sub_norm], penalty=pen, psi=(p0, p1, p2, p3), ub_start=ub_s, lb_end=lb_e, ub_end=ub_e,
               barcode_segm_events=e2, barcode_keep_events=keep)
    return seg, ref, bool(int(g[f"clip64_{k}"]))


def read(rng, n, embed=True, tail=None, flat_tail=False, n_lead=None):
    """A read of exactly `n` samples on the 1/8 grid: `n_lead` leader levels | the 84 consensus levels (random ones unless
    `embed`) | 30 barcode levels.  `tail`: samples of the 30 barcode levels together (default: their share of `n`);
    `flat_tail`: the barcode is ONE noise-free level -- its score curve is zero, so the tail has no peaks."""
    q = consensus()
    n_lead = int(rng.integers(4, 14)) if n_lead is None else n_lead
    lv = np.concatenate([rng.normal(0, 1, n_lead), q if embed else rng.normal(0, 1, q.size), rng.normal(0, 1, 30)]) * 12.0 + 85.0
    dw = rng.integers(14, 60, lv.size).astype(np.int64)
    head, bar = dw[:-30], dw[-30:]
    tail = int(n * bar.sum() / dw.sum()) if tail is None else int(tail)
    head = np.maximum(head * (n - tail) // int(head.sum()), 1)
    bar = np.maximum(bar * tail // int(bar.sum()), 1)
    head[0] += (n - tail) - int(head.sum())
    bar[-1] += tail - int(bar.sum())
    assert head[0] > 0 and bar[-1] > 0
    dw = np.concatenate([head, bar])
    x = np.repeat(lv, dw) + rng.normal(0, 1.5, n)
    if flat_tail:
        x[n - tail:] = 85.0
    assert x.size == n
    return (np.round(x * 8.0) / 8.0).astype(np.float32)


def quiet_row(rng, n, steps=60):
    """`steps` noise-free levels: about `steps` peaks, fewer than num_events -- "event segmentation failed" """
    cuts = np.sort(rng.choice(np.arange(200, n - 200, 40), steps - 1, replace=False))
    lv = np.round((85.0 + 12.0 * rng.normal(size=steps)) * 8.0) / 8.0
    return np.repeat(lv, np.diff(np.concatenate([[0], cuts, [n]]))).astype(np.float32)


def minibatch(rows):
    stride = max(r.size for r in rows)
    mb = np.full((len(rows), stride), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        mb[i, : r.size] = r
    return mb


def seg_params(**kw):
    return orc.SegParams(**{**dict(barcode_num_events=K, clip_bounds_f64=False, **SEG), **kw})


def refine_params(**kw):
    return orc.RefineParams(query=consensus(), **{**REF, **kw})


def oracle(b, rows=None, seg=None, ref=None):
    """(fpt, dwell, stats, idx, status) of the CPU oracle, which has no window limit"""
    return orc.fingerprint_refine_batch(b["rows"] if rows is None else rows, b["a_s"], b["a_e"], seg or seg_params(),
                                        ref or refine_params(), ok=b["ok"])


def expected(want, win):
    """the oracle's answer as the engine gives it with the option on: a window beyond 65 536 samples is "unknown" """
    fpt, dwell, stats, idx, status = (a.copy() for a in want)
    beyond = (np.asarray(win) > LONG_CAP) & (status != 1)
    status[beyond], fpt[beyond], dwell[beyond], stats[beyond], idx[beyond] = 5, np.nan, 0, np.nan, -1
    return fpt, dwell, stats, idx, status


def _bounds(mb, a_s, a_e):
    a_s, a_e = np.array(a_s, dtype=np.int32), np.array(a_e, dtype=np.int32)
    win = np.minimum(a_e.astype(np.int64) + PADDING, mb.shape[1]) - np.maximum(a_s.astype(np.int64) - PADDING, 0)
    return a_s, a_e, win


# the whole-row windows the edge batch starts with: the default cap (today's route), one beyond it, a multiple of 64 behind
# it, both sides of 32 768 (a thread's chunk of the state bytes goes from 32 to 33 positions), the long cap and one beyond
EDGE_LENGTHS = (16384, 16385, 16448, 32768, 32769, 65536, 65537)
I_TAIL_LONG, I_TAIL_SHORT, I_NO_CONS, I_FEW_PEAKS, I_FLAT_TAIL, I_NAN_TAIL, I_NAN_RUN, I_CROP, I_DEAD, I_NO_CONS2, I_SHORT = range(7, 18)


@functools.lru_cache(maxsize=None)
def edge_batch():
    """dict rows (n, stride) float32 with NaN tails, a_s, a_e, ok, win (the window each read's bounds select) -- read-only --
    and `want`, the oracle's (fpt, dwell, stats, idx, status) under the tRNA parameters (mean / mean normalisations)"""
    rng = np.random.default_rng(20261024)
    rows, a_s, a_e, ok = [], [], [], []

    def add(row, s=PADDING, e=None, good=1):
        rows.append(row)
        a_s.append(s)
        a_e.append(row.size - PADDING if e is None else e)
        ok.append(good)

    for n in EDGE_LENGTHS:
        add(read(rng, n))
    add(read(rng, 60000, tail=25000))                  # 7: slow barcode levels: the tail exceeds 16 384 samples
    add(read(rng, 56000, tail=3600))                   # 8: a short tail far out: sig_barcode_start beyond 50 000
    add(read(rng, 24000, embed=False))                 # 9: no consensus: status 6, stats and indices reported
    add(quiet_row(rng, 26000))                         # 10: too few peaks in the adapter pass: status 3
    add(read(rng, 30000, flat_tail=True, n_lead=36))   # 11: a flat barcode behind a long leader: too few peaks in the tail
    add(read(rng, 20000), e=20000 + 57)                # 12: a_end + padding beyond the samples: the NaN tail
    r = read(rng, 24000)
    r[12000:12004] = np.nan
    add(r)                                             # 13: a NaN run inside a long window
    add(read(rng, 40000), s=30)                        # 14: a_start < padding
    add(read(rng, 30000), good=0)                      # 15: ok = 0
    add(read(rng, 40000, embed=False))                 # 16: no consensus once more
    add(read(rng, 4000))                               # 17: an everyday read
    mb = minibatch(rows)
    a_s, a_e, win = _bounds(mb, a_s, a_e)
    b = dict(rows=mb, a_s=a_s, a_e=a_e, ok=np.array(ok, dtype=np.uint8), win=win)
    want = oracle(b)
    st, idx = want[4], want[3]
    # ---- the batch holds its edges, by the oracle's word ------------------------------------------------------------
    assert tuple(win[: len(EDGE_LENGTHS)]) == EDGE_LENGTHS
    long = (win > CAP) & (win <= LONG_CAP)
    assert (long & (st == 0)).sum() >= 6 and (long & (st == 6)).sum() >= 2, st
    assert st[0] in (0, 6) and st[5] == 0 and st[4] == 0, st       # 16 384 on today's route; 65 536 and 32 769 refine
    tail_len = win - idx[:, 2]
    assert st[I_TAIL_LONG] == 0 and tail_len[I_TAIL_LONG] > CAP, (st[I_TAIL_LONG], tail_len[I_TAIL_LONG])
    assert st[I_TAIL_SHORT] == 0 and idx[I_TAIL_SHORT, 2] > 50000 and tail_len[I_TAIL_SHORT] < 6000, idx[I_TAIL_SHORT]
    assert st[I_NO_CONS] == 6 and st[I_NO_CONS2] == 6 and np.isfinite(want[2][I_NO_CONS]).all() and (idx[I_NO_CONS] >= 0).all()
    assert st[I_FEW_PEAKS] == 3 and st[I_FLAT_TAIL] == 3, st[[I_FEW_PEAKS, I_FLAT_TAIL]]
    assert st[I_NAN_TAIL] not in (0, 1, 6) and st[I_NAN_RUN] not in (0, 1, 6), st[[I_NAN_TAIL, I_NAN_RUN]]
    assert a_s[I_CROP] < PADDING and st[I_CROP] in (0, 6) and st[I_DEAD] == 1 and st[I_SHORT] in (0, 6)
    assert int(a_e[I_NAN_TAIL]) + PADDING > 20000 and win[I_NAN_TAIL] == 20157
    for a in (*b.values(), *want):
        a.setflags(write=False)
    b["want"] = want
    return b


@functools.lru_cache(maxsize=None)
def ways_batch():
    """The 12 reads every way in is shown: eight long ones (16 385 .. 65 536 samples; one without the consensus, one
    with a barcode tail beyond 16 384 samples), three ordinary ones and a failed detection, quantised to int16
    (tests/helpers/adc_inputs.py) so that the float32 rows ARE `sig_proc.calibrate_adc` of the int16 rows.
    -> dict adc / row_len / offset / scale / rows / a_s / a_e / ok / padding, and `want`: the oracle on the float32 rows"""
    rng = np.random.default_rng(13)
    rows = [read(rng, 16385), read(rng, 20000), read(rng, 32769), read(rng, 49152), read(rng, 65536),
            read(rng, 24000, embed=False), read(rng, 60000, tail=25000), read(rng, 3000), read(rng, 30000),
            read(rng, 11201), read(rng, 17000), read(rng, 16384)]
    mb = minibatch(rows)
    assert mb.shape == (12, LONG_CAP)
    adc, row_len, offset, scale = adc_inputs.quantise(mb, 14)
    from warpdemux_amd import sig_proc

    cal = sig_proc.calibrate_adc(adc, row_len, offset, scale)
    a_s = np.full(12, PADDING, dtype=np.int32)
    a_e = (row_len - PADDING).astype(np.int32)
    a_s[7] = 30                                 # the padding is cropped
    a_e[10] = row_len[10] + 20                  # into the NaN tail: a window of 17 120 samples, 120 of them NaN
    ok = np.ones(12, dtype=np.uint8)
    ok[8] = 0
    b = dict(adc=adc, row_len=row_len, offset=offset, scale=scale, rows=cal, a_s=a_s, a_e=a_e, ok=ok, padding=PADDING)
    want = oracle(b)
    st = want[4]
    long = (np.minimum(a_e + PADDING, LONG_CAP) - np.maximum(a_s - PADDING, 0) > CAP) & (ok != 0)
    assert long.sum() == 8 and (st[long] == 0).sum() >= 5 and st[5] == 6 and st[8] == 1 and st[10] not in (0, 1, 6), st
    assert st[6] == 0 and (60000 - want[3][6, 2]) > CAP
    for a in (*b.values(), *want):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    b["want"] = want
    b["long"] = long
    return b
