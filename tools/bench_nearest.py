#!/usr/bin/env python3
"""What the nearest-reference rule (wdx_nearest_dev / wdx_demux_nearest_dev) costs against the calls it stands beside, on one
MI355X.  In one process, alternating after a warm-up call of each, every call bracketed by device events:

  (a) C3 shape, 10 references x 110 points, a shard of raw reads: `demux_nearest` without `dist` (the rule in the DTW kernel's
      epilogue, no distance written) against `demux` (argmin in the epilogue, the (n, 10) matrix written);
  (a-dtw) the DTW stage of (a) alone on the shard's fingerprints, and the same at 25 points (the unrolled kernel, held to three
      waves per SIMD with the rule in it): `nearest` without `dist` against `dtw` with its argmin;
  (b) R2 shape, 2 601 references x 25 points under 11 labels, 200 000 reads: `nearest` without `dist` (row blocks of at most
      96 MiB through the context's buffer) against `nearest` with `dist` (the full 2 GB matrix, then the row kernel).

Per variant: median / min / max ms per call and the spread (max - min) / median.  The calls of a pair are compared bit for bit
at the timed size.

    python tools/bench_nearest.py --out profiles/nearest_rule.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def timed(torch, fn, reps):
    """per-call ms of the variants in `fn` (name -> callable), alternating, after one warm-up call of each"""
    for f in fn.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fn}
    for _ in range(reps):
        for k, f in fn.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                "spread": (max(v) - min(v)) / statistics.median(v)} for k, v in ms.items()}


def route(eng):
    from warpdemux_amd import _lib

    i = eng.ctx.dtw_last_launch()
    return {"family": _lib.DTW_FAMILY_NAMES[i.family], "band_w": i.band_w, "layout": _lib.DTW_LAYOUT_NAMES[i.layout],
            "rule_fused": int(i.fused_argmin), "grid": [int(i.grid_x), int(i.grid_y)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shard-reads", type=int, default=1_000_000)
    ap.add_argument("--r2-reads", type=int, default=200_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from warpdemux_amd import sig_proc, synth
    from warpdemux_amd.engine import DemuxEngine

    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    rng = np.random.default_rng(1)

    # (a) raw rows -> call
    K, nY, n = 110, 10, args.shard_reads
    eng = DemuxEngine(np.zeros((nY, K)), 15, 0.1, sig_proc.SegParams(barcode_num_events=K))
    sig, off, a_s, a_e, _, max_len = eng.synth_packed(synth.SynthSpec(n_barcodes=nY), 0, n)
    fpt, _, _, st = eng.fingerprint(sig[: int(off[4096].item())], a_s[:4096], a_e[:4096], offsets=off[:4097], max_len=max_len,
                                    want_stats=False)
    good = np.flatnonzero(st.cpu().numpy() == 0)
    eng.set_refs(fpt.cpu().numpy()[good[:nY]], 15, 0.1)
    res = {}

    def demux():
        res["demux"] = eng.demux(sig, a_s, a_e, offsets=off, max_len=max_len, out=res.get("demux"), want_fpt=True)

    def demux_nearest():
        res["nearest"] = eng.demux_nearest(sig, a_s, a_e, offsets=off, max_len=max_len)

    t = timed(torch, {"demux": demux, "demux_nearest_no_dist": demux_nearest}, args.reps)
    demux_nearest()
    r = route(eng)
    torch.cuda.synchronize()
    same = bool(torch.equal(res["demux"].call, res["nearest"].call))
    out["a_c3_raw_rows"] = {"reads": n, "refs": nY, "L": K, "route": r, "calls_equal": same, **t}
    X = res["demux"].fpt
    t = timed(torch, {"dtw_argmin": lambda: eng.dtw(X), "nearest_no_dist": lambda: eng.nearest(X)}, args.reps)
    eng.nearest(X)
    out["a_c3_dtw_stage"] = {"reads": n, "refs": nY, "L": K, "route": route(eng), **t}
    del sig, res, X
    eng.close()

    # (a-dtw, 25 points)
    K = 25
    eng = DemuxEngine(rng.normal(size=(nY, K)), 15, 0.1, sig_proc.SegParams(barcode_num_events=K))
    X = torch.from_numpy(rng.normal(size=(n, K))).to(eng.tdev)
    t = timed(torch, {"dtw_argmin": lambda: eng.dtw(X), "nearest_no_dist": lambda: eng.nearest(X)}, args.reps)
    am, nr = eng.dtw(X)[1], eng.nearest(X)
    out["a_short_dtw_stage"] = {"reads": n, "refs": nY, "L": K, "route": route(eng), "calls_equal": bool(torch.equal(am, nr.call)), **t}
    del X
    eng.close()

    # (b) R2
    nY, n = 2601, args.r2_reads
    Y = rng.normal(size=(nY, K))
    eng = DemuxEngine(Y, 15, 0.1, sig_proc.SegParams(barcode_num_events=K))
    X = torch.from_numpy(Y[rng.integers(0, nY, size=n)] + 0.4 * rng.normal(size=(n, K))).to(eng.tdev)
    labels = torch.from_numpy((np.arange(nY) % 11).astype(np.int32)).to(eng.tdev)
    keep = {}

    def blocks():
        keep["blocks"] = eng.nearest(X, labels=labels, n_labels=11)

    def full():
        keep["full"] = eng.nearest(X, labels=labels, n_labels=11, want_dist=True)

    t = timed(torch, {"nearest_no_dist_row_blocks": blocks, "nearest_full_matrix_then_rows": full}, args.reps)
    blocks()
    r = route(eng)
    torch.cuda.synchronize()
    same = bool(torch.equal(keep["blocks"].call, keep["full"].call) and
                torch.equal(keep["blocks"].best.view(torch.int32), keep["full"].best.view(torch.int32)))
    out["b_r2"] = {"reads": n, "refs": nY, "L": K, "labels": 11, "route_of_the_last_block": r, "results_equal": same, **t}
    eng.close()

    print(json.dumps(out, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
