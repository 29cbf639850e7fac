#!/usr/bin/env python
"""Wall time of one live tick: p50 / p99 over --ticks ticks at 16, 128 and 512 reads.

  --what legacy   wdx_live_tick, DTW_SVM tail, float32 synthetic RNA004 rows.  Bound by hand to the five symbols it needs, so
                  --lib may name ANY build of libwdx_hip.so (an older one included): this is the A/B of the shared tick body.
  --what trna     the tRNA flow on reads that carry a consensus: ONE tick (refinement + boost tail) against the two host calls
                  that gave the same answer before it (sig_proc.fingerprint_refine_batch on a minibatch, then
                  Fpt_Boost.predict on the successful fingerprints); the minibatch is built outside the timed region, and
                  once more inside it (a live caller holds ragged rows, so it pays for the packing too).  The tick is timed
                  twice: `one_call` = LiveDemux.tick (Python marshalling of the rows and result copies included) and
                  `one_call_c_abi` = wdx_live_tick_ex itself, its pointer table and arrays built beforehand.
  --what adc      LiveDemux.tick_adc against LiveDemux.tick on the same reads (DTW_SVM model), int16 rows being the
                  quantisation of the float32 ones; each also at the C ABI (`*_c_abi`).
  --what aggregate  --raw FILE: the JSON lines of the runs above -> the summary committed as profiles/live_ex_latency.json
                  (printed; --out writes it).

One JSON line per measurement on stdout; --out appends them to a file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from warpdemux_amd import _lib, models, sig_proc, synth  # noqa: E402

K, SIZES = 25, (16, 128, 512)


def rna004_rows(n, first=40_000):
    sig, off, a_s, a_e, _ = synth.generate_packed(synth.SynthSpec(n_barcodes=4), first, n)
    rows = [sig[off[i]:off[i + 1]].copy() for i in range(n)]
    return rows, np.zeros(n, np.int32), np.array([r.size - 100 for r in rows], np.int32)


def consensus_rows(n, query, seed=7):
    """reads that carry `query` behind a short lead and a barcode tail behind it (the shape tests/helpers/refine_inputs.py
    gives its reads), 2 500 .. 6 000 samples"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        lv = np.concatenate([rng.normal(0, 1, int(rng.integers(2, 34))), query, rng.normal(0, 1, 30)]) * 12.0 + 85.0
        dw = rng.integers(12, 40, lv.size)
        rows.append((np.repeat(lv, dw) + rng.normal(0, 1.5, int(dw.sum()))).astype(np.float32))
    return rows, np.full(n, 100, np.int32), np.array([r.size - 100 for r in rows], np.int32)


def svm_model(k=4, n_train=300, seed=3):
    """parameters of a fitted SVC (precomputed kernel) on noisy copies of k centres; the kernel it is fitted on is a stand-in
    (Euclidean): only the shape of the model matters to a tick's wall time"""
    from sklearn.svm import SVC

    rng = np.random.default_rng(seed)
    y = np.arange(n_train) % k
    Xtr = rng.normal(size=(k, K))[y] + 0.6 * rng.normal(size=(n_train, K))
    Ktr = np.exp(-np.linalg.norm(Xtr[:, None] - Xtr[None], axis=2) / 5.0)
    svc = SVC(kernel="precomputed", probability=True, random_state=0).fit(Ktr, y)
    return models.DTW_SVM(Xtr, svc._n_support, svc.support_, svc._dual_coef_, -svc._intercept_, svc._probA, svc._probB,
                          {i: i + 1 for i in range(k)}, np.full(k, 0.2), 15, 0.1, block_size=500)


def boost_model(n_trees=200, depth=6, dim=4, seed=81):
    rng = np.random.default_rng(seed)
    trees = [(rng.integers(0, K, depth), rng.uniform(-1.5, 1.5, depth).astype(np.float32), [False] * depth,
              rng.normal(0, 0.2, (1 << depth, dim))) for _ in range(n_trees)]
    return models.Fpt_Boost(trees, K, 1.0, rng.normal(0, 0.5, dim), {i: i + 1 for i in range(dim)}, np.full(dim, 0.1))


def percentiles(fn, ticks, warmup):
    for _ in range(warmup):
        fn()
    t = np.empty(ticks)
    for i in range(ticks):
        t0 = time.perf_counter()
        fn()
        t[i] = time.perf_counter() - t0
    return {"p50_ms": round(float(np.percentile(t, 50)) * 1e3, 4), "p99_ms": round(float(np.percentile(t, 99)) * 1e3, 4)}


def c_abi_tick(ld, rows, a_s, a_e, offset=None, scale=None):
    """wdx_live_tick_ex on `ld`'s context with everything marshalled beforehand (status, call and the tail's outputs wanted,
    as `ld.tick(..., want_dist=False)` asks): a function that runs one tick, and the arrays it fills"""
    n = len(rows)
    adc = rows[0].dtype == np.int16
    ptrs = np.array([r.ctypes.data for r in rows], dtype=np.uintp)
    ln = np.array([r.size for r in rows], np.int32)
    o = dict(status=np.empty(n, np.int32), call=np.empty(n, np.int32), prob=np.empty((n, max(ld.k, 1))),
             pred=np.empty(n, np.int32), conf=np.empty(n))
    desc = _lib.LiveInC(None if adc else _lib.addr(ptrs), _lib.addr(ptrs) if adc else None, _lib.addr(offset), _lib.addr(scale),
                        _lib.addr(ln), n, _lib.addr(a_s), _lib.addr(a_e), None, ld.tail, 0)
    out = _lib.MinibatchOutC(_lib.addr(o["status"]), _lib.addr(o["call"]), None, None, None, None, _lib.addr(o["prob"]),
                             _lib.addr(o["pred"]), _lib.addr(o["conf"]))
    bad = C.c_int64(0)
    keep = (rows, ptrs, ln, a_s, a_e, offset, scale, o)   # everything the call reads or writes by address

    def tick(keep=keep):
        rc = ld.L.wdx_live_tick_ex(ld.ctx.handle, C.byref(desc), C.byref(ld._pc), None if ld._rc is None else C.byref(ld._rc),
                                   ld.nY, 0, C.byref(out), None, C.byref(bad))
        assert rc == 0

    return tick, o


def legacy(args):
    """wdx_live_tick of whatever library --lib names"""
    path = args.lib or _lib.LIB_PATH
    _lib._preload_hip_runtime()
    L = C.CDLL(path)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.wdx_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.wdx_ctx_destroy.argtypes = [vp]
    L.wdx_ctx_destroy.restype = None
    L.wdx_set_refs.argtypes = [vp, vp, i64, i64, i32, C.c_double]
    L.wdx_svm_set_model.argtypes = [vp, C.POINTER(_lib.SvmModelC)]
    L.wdx_live_tick.argtypes = [vp, vp, vp, i64, vp, vp, vp, C.POINTER(_lib.SegParamsC), i64, i32, vp, vp, vp, vp, vp, vp, vp]
    m = svm_model()
    h = vp()
    assert L.wdx_ctx_create(0, C.byref(h)) == 0
    assert L.wdx_set_refs(h, _lib.ptr(m._X), m._X.shape[0], K, 15, 0.1) == 0
    mc = m.to_c()
    assert L.wdx_svm_set_model(h, C.byref(mc)) == 0
    pc = sig_proc.SegParams(barcode_num_events=K).to_c()
    out = []
    for n in SIZES:
        rows, a_s, a_e = rna004_rows(n)
        ptrs = (vp * n)(*[r.ctypes.data for r in rows])
        ln = np.array([r.size for r in rows], np.int32)
        st, call, pred = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        prob, conf = np.empty((n, m.n_classes)), np.empty(n)

        def tick():
            rc = L.wdx_live_tick(h, ptrs, _lib.ptr(ln), n, _lib.ptr(a_s), _lib.ptr(a_e), None, C.byref(pc), m._X.shape[0], 1,
                                 None, None, _lib.ptr(call), _lib.ptr(st), _lib.ptr(prob), _lib.ptr(pred), _lib.ptr(conf))
            assert rc == 0

        rec = dict(what="legacy", lib=os.path.basename(os.path.dirname(path)) or path, label=args.label, reads=n,
                   ok_share=None, window_mbytes=round(sum(min(r.size, int(e) + 100) for r, e in zip(rows, a_e)) * 4 / 1e6, 2),
                   **percentiles(tick, args.ticks, args.warmup))
        rec["ok_share"] = round(float((st == 0).mean()), 3)
        out.append(rec)
    L.wdx_ctx_destroy(h)
    return out


def trna(args):
    from warpdemux_amd.live import LiveDemux

    query = np.random.default_rng(1).normal(size=84)
    hp = sig_proc.SegParams(barcode_num_events=K, padding=100, min_obs_per_base=9, running_stat_width=18, num_events=120)
    hr = sig_proc.RefineParams(query=query, barcode_segm_events=25, barcode_keep_events=K)
    bm = boost_model()
    ld = LiveDemux(model=bm, params=hp, refine=hr, max_reads=max(SIZES), max_samples=6500)
    out = []
    for n in SIZES:
        rows, a_s, a_e = consensus_rows(n, query)
        stride = max(r.size for r in rows)

        def pack():
            mb = np.full((n, stride), np.nan, dtype=np.float32)
            for i, r in enumerate(rows):
                mb[i, : r.size] = r
            return mb

        mb = pack()

        def two_calls(mb=mb):
            fb = sig_proc.fingerprint_refine_batch(mb, a_s, a_e, hp, hr)
            good = fb.status == 0
            return fb, bm.predict_raw(fb.fpt[good]) if good.any() else None

        one = ld.tick(rows, a_s, a_e, want_dist=False)
        fb, pr = two_calls()
        good = fb.status == 0
        assert np.array_equal(one.status, fb.status) and np.array_equal(one.prob[good], pr[1]), "the two ways disagree"
        raw, ro = c_abi_tick(ld, rows, a_s, a_e)
        raw()
        assert np.array_equal(ro["status"], one.status) and np.array_equal(ro["prob"], one.prob, equal_nan=True)
        t1 = percentiles(lambda: ld.tick(rows, a_s, a_e, want_dist=False), args.ticks, args.warmup)
        t0 = percentiles(raw, args.ticks, args.warmup)
        t2 = percentiles(two_calls, args.ticks, args.warmup)
        t3 = percentiles(lambda: two_calls(pack()), args.ticks, args.warmup)
        out.append(dict(what="trna", label=args.label, reads=n, ok_share=round(float(good.mean()), 3),
                        window_mbytes=round(sum(r.size for r in rows) * 4 / 1e6, 2), one_call=t1, one_call_c_abi=t0,
                        two_calls=t2, two_calls_with_pack=t3, ratio_p50=round(t1["p50_ms"] / t2["p50_ms"], 3),
                        ratio_p50_c_abi=round(t0["p50_ms"] / t2["p50_ms"], 3),
                        ratio_p50_with_pack=round(t1["p50_ms"] / t3["p50_ms"], 3)))
    ld.close()
    return out


def adc(args):
    from warpdemux_amd.live import LiveDemux

    m = svm_model()
    ld = LiveDemux(model=m, max_reads=max(SIZES), max_samples=9000)
    out = []
    for n in SIZES:
        rows, a_s, a_e = rna004_rows(n)
        rng = np.random.default_rng(5)
        scale = (0.1755 * (1.0 + 0.02 * rng.uniform(-1, 1, n))).astype(np.float32)
        offset = (-240.0 + rng.uniform(-20, 20, n)).astype(np.float32)
        q = [np.clip(np.rint(r.astype(np.float64) / float(s) - float(o)), -32768, 32767).astype(np.int16)
             for r, s, o in zip(rows, scale, offset)]
        f = [s * (x.astype(np.float32) + o) for x, s, o in zip(q, scale, offset)]     # the rows the int16 ones stand for
        a, b = ld.tick(f, a_s, a_e, want_dist=False), ld.tick_adc(q, offset, scale, a_s, a_e, want_dist=False)
        assert np.array_equal(a.status, b.status) and np.array_equal(a.prob, b.prob, equal_nan=True), "int16 and float32 ticks disagree"
        tf = percentiles(lambda: ld.tick(f, a_s, a_e, want_dist=False), args.ticks, args.warmup)
        ti = percentiles(lambda: ld.tick_adc(q, offset, scale, a_s, a_e, want_dist=False), args.ticks, args.warmup)
        cf = percentiles(c_abi_tick(ld, f, a_s, a_e)[0], args.ticks, args.warmup)
        ci = percentiles(c_abi_tick(ld, q, a_s, a_e, offset, scale)[0], args.ticks, args.warmup)
        out.append(dict(what="adc", label=args.label, reads=n, ok_share=round(float((a.status == 0).mean()), 3),
                        window_mbytes_float32=round(sum(min(r.size, int(e) + 100) for r, e in zip(f, a_e)) * 4 / 1e6, 2),
                        float32=tf, int16=ti, float32_c_abi=cf, int16_c_abi=ci, ratio_p50=round(ti["p50_ms"] / tf["p50_ms"], 3),
                        ratio_p50_c_abi=round(ci["p50_ms"] / cf["p50_ms"], 3)))
    ld.close()
    return out


def aggregate(args):
    """the raw lines of one session -> one record: (a) parent and this tree side by side with the parent's run-to-run spread,
    (b) and (c) as measured"""
    import statistics

    recs = [json.loads(ln) for ln in open(args.raw) if ln.startswith("{")]
    out = {"tool": "tools/bench_live.py", "unit": "ms wall time per tick, host to host", "a_wdx_live_tick_svm_float32": {},
           "b_trna_flow": {}, "c_int16_vs_float32": {}}
    for n in SIZES:
        leg = [r for r in recs if r["what"] == "legacy" and r["reads"] == n]
        par = [r for r in leg if r["label"].startswith("parent")]
        new = [r for r in leg if not r["label"].startswith("parent")]
        if par and new:
            pp, nn = [r["p50_ms"] for r in par], [r["p50_ms"] for r in new]
            out["a_wdx_live_tick_svm_float32"][str(n)] = {
                "parent_p50": pp, "parent_p99": [r["p99_ms"] for r in par], "new_p50": nn, "new_p99": [r["p99_ms"] for r in new],
                "parent_median_p50": statistics.median(pp), "parent_spread_p50": round(max(pp) - min(pp), 4),
                "new_median_p50": statistics.median(nn),
                "new_within_parent_spread_or_faster": statistics.median(nn) <= statistics.median(pp) + (max(pp) - min(pp))}
        for what, key in (("trna", "b_trna_flow"), ("adc", "c_int16_vs_float32")):
            for r in recs:
                if r["what"] == what and r["reads"] == n:
                    out[key][str(n)] = {k: v for k, v in r.items() if k not in ("what", "label", "reads")}
    return [out]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=("legacy", "trna", "adc", "aggregate"), required=True)
    ap.add_argument("--raw", default=None, help="aggregate: the file of JSON lines to summarise")
    ap.add_argument("--lib", default=None, help="legacy only: the libwdx_hip.so to measure (default: this tree's)")
    ap.add_argument("--label", default="")
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    recs = {"legacy": legacy, "trna": trna, "adc": adc, "aggregate": aggregate}[args.what](args)
    for r in recs:
        line = json.dumps(r, indent=1 if args.what == "aggregate" else None)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
