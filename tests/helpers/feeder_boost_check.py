"""Run by tests/test_gpu_boost_paths.py in a FRESH interpreter (the parent of a Feeder must not have touched the GPU):
Feeder(model=Fpt_Boost, refs=None) served to four forked workers -- a refine ring and a plain ring, float32 rows, then
int16 rows --, `predict(X)` through wdx_feeder_predict_boost, and a ring whose n_classes is not the model's k, which must
answer every minibatch WDX_ERR_INVALID and keep serving.  The yardstick is the direct calls (`sig_proc.fingerprint_batch` /
`fingerprint_refine_batch`, then `Fpt_Boost.predict_raw` on the successful fingerprints), made once in a child process of
its own.  Every output bit for bit, NaN-aware.  Prints one JSON line."""
import json
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from helpers import boost_ref, refine_inputs as ri  # noqa: E402
from warpdemux_amd import models, sig_proc  # noqa: E402
from warpdemux_amd.feeder import Feeder  # noqa: E402

SEEDS = (101, 202)
K = 25
HP = sig_proc.SegParams(barcode_num_events=K, **ri.SEG)
HR = sig_proc.RefineParams(query=ri.consensus(), **ri.REF)
# worker w: (seed, NaN inside a window)
JOBS = [(SEEDS[0], True), (SEEDS[1], False), (SEEDS[1], True), (SEEDS[0], False)]
BATCH = {s: ri.batch(s) for s in SEEDS}
FEEDERS = {}     # inherited by the forked workers
LABELS = {0: 7, 1: 1, 2: 10, 3: 4}


def boost_model(dim=4):
    m = boost_ref.random_model(65, 6, dim, K, seed=81)
    trees = [(f, b, [False] * len(f), lv) for f, b, lv in m.trees]
    lm = LABELS if dim == 4 else {i: i for i in range(m.k)}
    return models.Fpt_Boost(trees, K, m.scale, m.bias, lm, np.array([0.05, 0.2, 0.1, 0.3]) if dim == 4 else None)


MODEL = boost_model()


def same(a, b):
    return bool(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def yardstick(_):
    """(a GPU-facing child of its own) the direct calls on every variant: {(refine, seed, nan): (fb, y_pred, y_prob)}"""
    out = {}
    for refine in (True, False):
        for seed in SEEDS:
            b = BATCH[seed]
            for nan in (False, True):
                rows = b["rows_nan" if nan else "rows"]
                fb = (sig_proc.fingerprint_refine_batch(rows, b["a_s"], b["a_e"], HP, HR, success=b["ok"]) if refine
                      else sig_proc.fingerprint_batch(rows, b["a_s"], b["a_e"], HP, success=b["ok"]))
                _, prob, pred, _conf = MODEL.predict_raw(fb.fpt[fb.status == 0])
                out[(refine, seed, nan)] = (fb, pred, prob)
    return out


def worker(w):
    """one forked worker: its minibatch through the feeder (no context, no HIP call here), then `predict` of its own
    successful fingerprints"""
    seed, nan = JOBS[w]
    b = BATCH[seed]
    f, adc = FEEDERS["now"]
    if adc:
        fb, (y_pred, y_prob) = f.detect_and_predict_adc(b["adc"], b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"],
                                                        success=b["ok"])
    else:
        fb, (y_pred, y_prob) = f.detect_and_predict(b["rows_nan" if nan else "rows"], b["a_s"], b["a_e"], success=b["ok"])
    p_pred, p_prob = f.predict(fb.fpt[fb.status == 0])
    return fb, y_pred, y_prob, p_pred, p_prob


def compare(res, want, refine):
    fb, y_pred, y_prob, p_pred, p_prob = res
    wf, w_pred, w_prob = want
    return {"status": same(fb.status, wf.status), "fpt": same(fb.fpt, wf.fpt), "dwell": same(fb.dwell, wf.dwell),
            "stats": same(fb.stats, wf.stats),
            "refine_idx": (same(fb.refine_idx, wf.refine_idx) if refine else fb.refine_idx is None),
            "y_pred": same(y_pred, w_pred), "y_prob": same(y_prob, w_prob), "predict_pred": same(p_pred, w_pred),
            "predict_prob": same(p_prob, w_prob)}


def code(call):
    try:
        call()
        return "served"
    except ValueError:
        return "INVALID"
    except Exception as e:  # noqa: BLE001
        return type(e).__name__


if __name__ == "__main__":
    ctx = mp.get_context("fork")
    with ctx.Pool(1) as pool:
        ref = pool.map(yardstick, [0])[0]
    rec = {"gpu_processes": 1, "refused": {}}
    n = BATCH[SEEDS[0]]["rows"].shape[0]
    stride = max(BATCH[s]["rows"].shape[1] for s in SEEDS)
    geo = dict(params=HP, max_reads=n, stride=stride, n_slots=4)
    for adc in (False, True):
        with Feeder(model=MODEL, refine=HR, adc=adc, **geo) as fr, Feeder(model=MODEL, adc=adc, **geo) as fp:
            rec["gpu_processes"] += 2
            for refine, f in ((True, fr), (False, fp)):
                FEEDERS["now"] = (f, adc)
                with ctx.Pool(4) as pool:
                    res = pool.map(worker, range(4), chunksize=1)
                name = f"{'refine' if refine else 'plain'} {'int16' if adc else 'float32'}"
                rec[name] = {f"w{w} {k}": v for w, r in enumerate(res)
                             for k, v in compare(r, ref[(refine, JOBS[w][0], JOBS[w][1] and not adc)], refine).items()}
            if not adc:
                # `predict` on more rows than a slot holds, return_df included; demux_batch has nothing to compare against
                fb, w_pred, w_prob = ref[(True, SEEDS[0], False)]
                X = np.tile(fb.fpt[fb.status == 0], (3, 1))
                y_pred, y_prob = fr.predict(X)
                df = fp.predict(X[:20], return_df=True)
                rec["predict"] = {"pred": same(y_pred, np.tile(w_pred, 3)), "prob": same(y_prob, np.tile(w_prob, (3, 1))),
                                  "more_than_a_slot": len(X) > n, "int64": y_pred.dtype == np.int64,
                                  "df": list(df.columns[:2]) == ["predicted_barcode", "confidence_score"] and
                                  bool(np.array_equal(df["predicted_barcode"].to_numpy(), w_pred[:20]))}
                b = BATCH[SEEDS[0]]
                # the fingerprints alone from both rings (the plain ring without references asks for the tail and drops it)
                for refine, f in ((True, fr), (False, fp)):
                    fo, wf = f.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], success=b["ok"]), ref[(refine, SEEDS[0], False)][0]
                    rec["predict"][f"fingerprints_only refine={refine}"] = bool(
                        same(fo.status, wf.status) and same(fo.fpt, wf.fpt) and same(fo.dwell, wf.dwell) and same(fo.stats, wf.stats))
                try:
                    fp.demux_batch(b["rows"], b["a_s"], b["a_e"], success=b["ok"])
                    rec["refused"]["demux_without_references"] = False
                except ValueError as e:
                    rec["refused"]["demux_without_references"] = "fingerprint-only" in str(e)
    del FEEDERS["now"]
    # A ring laid out for another class count than the resident model's: the ring (and the workers' outputs) are sized for 4
    # classes, the model the server holds has 3.  Feeder derives the ring's n_classes from its model, so the geometry is
    # patched for the time this one feeder is created.
    wrong = boost_model(3)
    import warpdemux_amd.feeder as fmod

    real_geo = fmod._lib.FeederGeometryC

    def geo_with_four_classes(n_slots, n_events, n_classes, *rest):
        return real_geo(n_slots, n_events, 4, *rest)

    fmod._lib.FeederGeometryC = geo_with_four_classes
    try:
        with Feeder(model=wrong, refine=HR, **geo) as odd:   # (a refine ring: it serves fingerprints without the tail)
            rec["gpu_processes"] += 1
            odd.n_classes = 4
            b = BATCH[SEEDS[0]]
            run = lambda: odd.detect_and_predict(b["rows"], b["a_s"], b["a_e"], success=b["ok"])   # noqa: E731
            rec["mismatch"] = {"first": code(run), "second": code(run),
                               "predict": code(lambda: odd.predict(np.zeros((2, K))))}
            fbo = odd.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], success=b["ok"])
            rec["mismatch"]["still_serving"] = bool(odd.alive() and same(fbo.fpt, ref[(True, SEEDS[0], False)][0].fpt))
    finally:
        fmod._lib.FeederGeometryC = real_geo
    print(json.dumps(rec))
