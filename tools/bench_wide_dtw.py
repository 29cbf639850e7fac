#!/usr/bin/env python3
"""What the wide-window DTW kernel (WDX_OPT_WIDE_DTW) costs against the scratch-row kernel it replaces, on one MI355X.

For each shape (L, window, nY, nX) one `DemuxEngine` holds the references and seeded float64 rows on the device; in one process
`engine.dtw` runs with the option off (scratch rows: the default route) and on (wide kernel), alternating, after one warm-up call
of each.  Every call is bracketed by device events and followed by a synchronise; recorded per route: median / min / max ms per
call over the repetitions, the spread (max - min) / median, and useful cell-updates/s (pairs x cells inside the band / median).
The two routes' distances and argmin are compared bit for bit at the timed size.  As context, not as a condition: the same rows
against the same references at window 32 (`band<32>`), with its own cell count.

    python tools/bench_wide_dtw.py --out profiles/wide_dtw.json
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

# (L, window, nY, nX, what the shape stands for)
SHAPES = [
    (110, None, 10, 1_000_000, "R1 references unbanded, a shard"),
    (110, None, 10, 1_000, "a minibatch"),
    (110, None, 10, 64, "a live tick"),
    (40, 33, 10, 1_000_000, "the narrowest wide window"),
    (254, None, 4, 100_000, "the longest fingerprint"),
    (64, None, 851, 4_096, "many references"),
    (110, None, 851, 16, "a few reads against many references (refs as lanes)"),
]


def band_cells(L, w):
    """cells (i, j) of the L x L matrix with |i - j| <= w - 1"""
    w = L if (w is None or w <= 0 or w > L) else w
    return L * L - (L - w) * (L - w + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternations after the warm-up")
    ap.add_argument("--max-reads", type=int, default=0, help="cap nX of every shape (0 = as listed; a rehearsal)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from warpdemux_amd import _lib
    from warpdemux_amd.engine import DemuxEngine

    dev = torch.device("cuda", 0)

    def timed(engine, X, out):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        engine.dtw(X, out=out)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def route(engine):
        i = engine.ctx.dtw_last_launch()
        return {"family": _lib.DTW_FAMILY_NAMES[i.family], "band_w": i.band_w, "layout": _lib.DTW_LAYOUT_NAMES[i.layout],
                "fused_argmin": bool(i.fused_argmin), "launches": i.launches, "refs_per_block": i.refs_per_block,
                "grid": [i.grid_x, i.grid_y]}

    def stats(ms, cells):
        med = statistics.median(ms)
        return {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "spread": (max(ms) - min(ms)) / med,
                "cell_updates_per_s": cells / (med * 1e-3)}

    results = []
    for L, window, nY, nX, what in SHAPES:
        if args.max_reads:
            nX = min(nX, args.max_reads)
        rng = np.random.default_rng(L * 1000 + nY)
        Y = rng.normal(size=(nY, L))
        g = torch.Generator(device=dev)
        g.manual_seed(nX + L)
        X = torch.randn((nX, L), generator=g, device=dev, dtype=torch.float64)
        engine = DemuxEngine(Y, window=window, penalty=0.1, device=0)
        outs = {k: (torch.empty((nX, nY), dtype=torch.float32, device=dev), torch.empty(nX, dtype=torch.int32, device=dev))
                for k in ("scratch", "wide")}
        ms = {"scratch": [], "wide": []}
        routes = {}
        for rep in range(-1, args.reps):        # (rep -1: the warm-up of both routes -- allocations, code upload)
            for k, on in (("scratch", 0), ("wide", 1)):
                engine.ctx.set_option(_lib.OPT_WIDE_DTW, on)
                t = timed(engine, X, outs[k])
                routes[k] = route(engine)
                if rep >= 0:
                    ms[k].append(t)
        engine.ctx.set_option(_lib.OPT_WIDE_DTW, 0)
        assert routes["scratch"]["family"] == "scratch" and routes["wide"]["family"] == "wide", routes
        same = bool(torch.equal(outs["scratch"][0].view(torch.int32), outs["wide"][0].view(torch.int32)) and
                    torch.equal(outs["scratch"][1], outs["wide"][1]))
        cells = nX * nY * band_cells(L, window)
        rec = {"L": L, "window": window, "nY": nY, "nX": nX, "what": what, "cells_per_call": cells,
               "scratch": dict(stats(ms["scratch"], cells), route=routes["scratch"]),
               "wide": dict(stats(ms["wide"], cells), route=routes["wide"]), "outputs_bitwise_equal": same}
        rec["speedup_median"] = rec["scratch"]["ms_median"] / rec["wide"]["ms_median"]
        # the condition: faster by more than the run-to-run spread -- the slowest wide call beats the fastest scratch call
        rec["wide_faster_beyond_spread"] = rec["wide"]["ms_max"] < rec["scratch"]["ms_min"]
        # context: band<32> on the same rows (window 32), its own cell count
        del engine
        eb = DemuxEngine(Y, window=32, penalty=0.1, device=0)
        tb = [timed(eb, X, outs["wide"]) for _ in range(args.reps + 1)][1:]
        cb = nX * nY * band_cells(L, 32)
        rec["band32_context"] = dict(stats(tb, cb), route=route(eb), cells_per_call=cb)
        del eb, outs, X
        torch.cuda.empty_cache()
        results.append(rec)
        print(json.dumps(rec), flush=True)

    doc = {"tool": "tools/bench_wide_dtw.py", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "timing": "device events around engine.dtw + synchronise, routes alternating in one process after one warm-up each",
           "condition": "wide_faster_beyond_spread: max ms of the wide route < min ms of the scratch route",
           "shapes": results}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    ok = all(r["outputs_bitwise_equal"] and r["wide_faster_beyond_spread"] for r in results)
    print("condition holds at every shape" if ok else "CONDITION FAILS at some shape")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
