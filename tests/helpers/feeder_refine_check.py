"""Run by tests/test_gpu_refine_paths.py in a FRESH interpreter (the parent of a Feeder must not have touched the GPU):
Feeder(refine=...) served to four forked workers -- float32 rows, then int16 rows --, a fingerprint-only feeder without
references, and a plain Feeder beside them.  The yardstick is the blocking call (`sig_proc.fingerprint_refine_batch`,
`sig_proc.fingerprint_batch`, `parallel_distances.nearest_reference`), made once in a child process of its own.  Every
output bit for bit, NaN-aware.  Prints one JSON line."""
import json
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from helpers import refine_inputs as ri  # noqa: E402
from warpdemux_amd import sig_proc  # noqa: E402
from warpdemux_amd.feeder import Feeder  # noqa: E402

SEEDS = (101, 202)
N_REFS, K = 16, 25
HP = sig_proc.SegParams(barcode_num_events=K, **ri.SEG)
HR = sig_proc.RefineParams(query=ri.consensus(), **ri.REF)
# worker w: (seed, NaN inside a window)
JOBS = [(SEEDS[0], True), (SEEDS[1], False), (SEEDS[1], True), (SEEDS[0], False)]
BATCH = {s: ri.batch(s) for s in SEEDS}
FEEDERS = {}     # inherited by the forked workers


def same(a, b):
    return bool(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True))


def yardstick(_):
    """(a GPU-facing child of its own) the blocking calls on every variant, the references, the plain fingerprints"""
    from warpdemux_amd import parallel_distances as pdist

    out = {}
    for seed in SEEDS:
        b = BATCH[seed]
        for nan in (False, True):
            out[(seed, nan)] = sig_proc.fingerprint_refine_batch(b["rows_nan" if nan else "rows"], b["a_s"], b["a_e"], HP, HR,
                                                                 success=b["ok"])
    f0 = out[(SEEDS[0], False)]
    refs = np.ascontiguousarray(f0.fpt[f0.status == 0][:N_REFS])
    for key, fb in list(out.items()):
        ok = fb.status == 0
        D, am = pdist.nearest_reference(fb.fpt[ok], refs, 15, 0.1)
        dist = np.full((ok.size, N_REFS), np.nan, dtype=np.float32)
        call = np.full(ok.size, -1, dtype=np.int32)
        dist[ok], call[ok] = D, am
        out[key] = (fb, dist, call)
    b = BATCH[SEEDS[0]]
    plain = sig_proc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], HP, success=b["ok"])
    return out, refs, plain


def worker(w):
    """one forked worker: its minibatch through the feeder (no context, no HIP call here)"""
    seed, nan = JOBS[w]
    b = BATCH[seed]
    if "int16" in FEEDERS:
        f = FEEDERS["int16"]
        cal = (b["row_len"], b["offset"], b["scale"])
        fb = f.fingerprint_batch_adc(b["adc"], *cal, b["a_s"], b["a_e"], success=b["ok"])
        dm = f.demux_batch_adc(b["adc"], *cal, b["a_s"], b["a_e"], success=b["ok"])
    else:
        f = FEEDERS["float32"]
        rows = b["rows_nan" if nan else "rows"]
        fb = f.fingerprint_batch(rows, b["a_s"], b["a_e"], success=b["ok"])
        dm = f.demux_batch(rows, b["a_s"], b["a_e"], success=b["ok"])
    return fb, dm


def compare(fb, dm, want):
    wf, dist, call = want
    return {"status": same(fb.status, wf.status), "fpt": same(fb.fpt, wf.fpt), "dwell": same(fb.dwell, wf.dwell),
            "stats": same(fb.stats, wf.stats), "refine_idx": fb.refine_idx is not None and same(fb.refine_idx, wf.refine_idx),
            "demux_status": same(dm.status, wf.status), "call": same(dm.call, call), "dist": same(dm.dist, dist)}


if __name__ == "__main__":
    ctx = mp.get_context("fork")
    with ctx.Pool(1) as pool:
        ref, refs, plain_ref = pool.map(yardstick, [0])[0]
    rec = {"gpu_processes": 1, "refused": {}}
    try:
        for seed in SEEDS:
            ri.check_kinds(ref[(seed, True)][0].status, True)
            ri.check_kinds(ref[(seed, False)][0].status, False)
        rec["kinds_ok"] = True
    except AssertionError as e:
        rec["kinds_ok"] = str(e)
    n, stride = BATCH[SEEDS[0]]["rows"].shape
    stride = max(BATCH[s]["rows"].shape[1] for s in SEEDS)
    geo = dict(params=HP, max_reads=n, stride=stride, n_slots=4)
    # float32 rows: four forked workers on a refine feeder, a plain feeder beside it
    with Feeder(refs=refs, window=15, penalty=0.1, refine=HR, **geo) as f32, \
            Feeder(refs=refs, window=15, penalty=0.1, **geo) as plain:
        rec["gpu_processes"] += 2
        FEEDERS["float32"] = f32
        with ctx.Pool(4) as pool:
            res = pool.map(worker, range(4), chunksize=1)
        rec["float32"] = {f"w{w} {k}": v for w, (fb, dm) in enumerate(res) for k, v in compare(fb, dm, ref[JOBS[w]]).items()}
        b = BATCH[SEEDS[0]]
        pf = plain.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], success=b["ok"])
        rec["plain"] = {"status": same(pf.status, plain_ref.status), "fpt": same(pf.fpt, plain_ref.fpt),
                        "dwell": same(pf.dwell, plain_ref.dwell), "stats": same(pf.stats, plain_ref.stats),
                        "no_refine_idx": pf.refine_idx is None, "differs_from_refine": not same(pf.fpt, ref[(SEEDS[0], False)][0].fpt)}
        try:
            f32.predict(np.zeros((2, K)))
            rec["refused"]["predict_without_model"] = False
        except ValueError as e:
            rec["refused"]["predict_without_model"] = "without a model" in str(e)
    del FEEDERS["float32"]
    # int16 rows (no NaN inside a window: int16 holds none)
    with Feeder(refs=refs, window=15, penalty=0.1, refine=HR, adc=True, **geo) as f16:
        rec["gpu_processes"] += 1
        FEEDERS["int16"] = f16
        with ctx.Pool(4) as pool:
            res = pool.map(worker, range(4), chunksize=1)
        rec["int16"] = {f"w{w} {k}": v for w, (fb, dm) in enumerate(res)
                        for k, v in compare(fb, dm, ref[(JOBS[w][0], False)]).items()}
    del FEEDERS["int16"]
    # no references, no model: fingerprints only
    with Feeder(refine=HR, **geo) as solo:
        rec["gpu_processes"] += 1
        b = BATCH[SEEDS[1]]
        fb = solo.fingerprint_batch(b["rows_nan"], b["a_s"], b["a_e"], success=b["ok"])
        wf = ref[(SEEDS[1], True)][0]
        rec["fingerprint_only"] = {"status": same(fb.status, wf.status), "fpt": same(fb.fpt, wf.fpt), "dwell": same(fb.dwell, wf.dwell),
                                   "stats": same(fb.stats, wf.stats), "refine_idx": same(fb.refine_idx, wf.refine_idx)}
        try:
            solo.demux_batch(b["rows"], b["a_s"], b["a_e"], success=b["ok"])
            rec["refused"]["demux_on_fingerprint_only"] = False
        except ValueError as e:
            rec["refused"]["demux_on_fingerprint_only"] = "fingerprint-only" in str(e)
    print(json.dumps(rec))
