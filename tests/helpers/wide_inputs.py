"""Inputs of tests/test_gpu_wide_dtw.py and tests/helpers/feeder_wide_check.py: synthetic reads (warpdemux_amd/synth.py, as
tests/helpers/adc_inputs.main_batch draws and quantises them: failed and garbage detections, inverted windows, windows into
the NaN tail) for the fused entries and the host ways in, and tRNA-like reads whose barcode tail is long enough for 40-event
fingerprints for the refining entries.  Large batches repeat the rows of the small one: the DTW sees the same fingerprints in
other lanes, waves and layouts, and the host generates a few hundred reads only."""
import functools

import numpy as np

from helpers import adc_inputs, refine_inputs as ri
from warpdemux_amd import sig_proc

REFINE_K = 40
REFINE_SEG = dict(ri.SEG)
REFINE_REF = dict(barcode_segm_events=REFINE_K, barcode_keep_events=REFINE_K)


@functools.lru_cache(maxsize=None)
def synth_batch(n=300):
    """adc_inputs.main_batch plus its calibrated float32 rows"""
    b = dict(adc_inputs.main_batch(n=n))
    b["rows"] = sig_proc.calibrate_adc(b["adc"], b["row_len"], b["offset"], b["scale"])
    return b


@functools.lru_cache(maxsize=None)
def refine_batch(seed=404, n=96):
    """helpers.refine_inputs.batch with 46 events behind the consensus instead of 30 (the refined barcode tail is cut into 40
    events), otherwise the same kinds of reads: a failed detection, a window far too short, reads without the consensus"""
    q = ri.consensus()
    rng = np.random.default_rng(seed)
    reads, lead = [], []
    for i in range(n):
        emb = i % 6 != 4
        lv = np.concatenate([rng.normal(0, 1, int(rng.integers(2, 34))), q if emb else rng.normal(0, 1, q.size),
                             rng.normal(0, 1, 46)]) * 12.0 + 85.0
        dw = rng.integers(12, 40, lv.size)
        x = np.repeat(lv, dw) + rng.normal(0, rng.uniform(0.8, 3.0), int(dw.sum()))
        junk = int(rng.integers(0, 1200))
        reads.append(np.concatenate([rng.normal(85, 12, junk), x]).astype(np.float32))
        lead.append(junk)
    sizes = np.array([r.size for r in reads])
    stride = int(sizes.max()) + 200
    mb = np.full((n, stride), np.nan, dtype=np.float32)
    for i, r in enumerate(reads):
        mb[i, : r.size] = r
    adc, row_len, offset, scale = adc_inputs.quantise(mb, seed + 1)
    a_s = np.array(lead, dtype=np.int32) + ri.PADDING
    a_e = (sizes - ri.PADDING).astype(np.int32)
    ok = np.ones(n, dtype=np.uint8)
    ok[ri.I_DEAD] = 0
    a_e[ri.I_SHORT] = a_s[ri.I_SHORT] + 900
    rows = sig_proc.calibrate_adc(adc, row_len, offset, scale)
    return dict(adc=adc, row_len=row_len, offset=offset, scale=scale, rows=rows, a_s=a_s, a_e=a_e, ok=ok, padding=ri.PADDING)


def tiled(b, n):
    """the batch's reads repeated up to n reads"""
    idx = np.arange(n) % len(b["a_s"])
    return {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) else v) for k, v in b.items()}


def host_refs(K=110, nY=10):
    """references every process of the host-way tests draws alike (a feeder's parent must not touch the GPU for them)"""
    return np.random.default_rng(610).normal(size=(nY, K))
