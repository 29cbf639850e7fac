#!/usr/bin/env python3
"""What barycenter reference signals cost on one MI355X, alternating in one process:

  band      `DemuxEngine.dba_step` as shipped at window 15: the band in registers, one lane per row (wdx_dba.hip)
  general   the same call with WDX_OPT_DBA_GENERAL = 1: two rolling rows per lane in global memory
  distance  the lower bound a path-producing step can be compared with -- what the API without this entry needs for the DISTANCES
            of the same (row, centre) pairs: `set_refs(centres)` plus `DemuxEngine.dtw` label by label (fused cells, no codes, no
            walk, no sums; each row against every centre, as that API computes them)

Shapes: 10 labels x 3 000 rows at (L 110, window 15), 4 labels x 900 rows at (25, 15), one label of 32 768 rows at (110, 15);
penalty 0.1.  Every call is bracketed by device events and followed by a synchronise; a warm-up of every route precedes the timed
alternation; per route: median / min / max ms over 25 alternations and the spread (max - min) / median.  The clocks are left as found (nothing is set).
band and general are compared bit for bit at the timed size.  Then a 10-step `DemuxEngine.barycenters` on the first shape, and
the `nearest` error rate on held-out rows with the barycenters as references against the rate with the medoids (noisier rows
than the timing's, so that there are errors to count).

    python tools/bench_dba.py --out profiles/dba.json
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

# (labels, rows per label, L, window, penalty)
SHAPES = [(10, 3000, 110, 15, 0.1), (4, 900, 25, 15, 0.1), (1, 32768, 110, 15, 0.1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25, help="alternations after the warm-up")
    ap.add_argument("--max-rows", type=int, default=0, help="cap the rows per label (0 = as listed; a rehearsal)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from warpdemux_amd import _lib
    from warpdemux_amd.engine import DemuxEngine

    dev = torch.device("cuda", 0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def make(G, m, L, noise, seed):
        gen = torch.Generator(device=dev).manual_seed(seed)
        truth = torch.randn((G, L), generator=gen, device=dev, dtype=torch.float64).cumsum(dim=1) * 0.3
        lab = np.repeat(np.arange(G, dtype=np.int32), m)
        np.random.default_rng(G).shuffle(lab)
        X = (truth[torch.from_numpy(lab.astype(np.int64)).to(dev)] + noise * torch.randn((len(lab), L), generator=gen, device=dev, dtype=torch.float64))
        return X.contiguous(), lab, gen, truth

    def stats(v):
        med = statistics.median(v)
        return dict(median_ms=round(med, 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), spread=round((max(v) - min(v)) / med, 4))

    results = []
    first = None
    for G, m, L, window, penalty in SHAPES:
        if args.max_rows:
            m = min(m, args.max_rows)
        X, lab, gen, _ = make(G, m, L, 0.35, 1000 * L + G)
        rows_of = [torch.from_numpy(np.flatnonzero(lab == g)).to(dev) for g in range(G)]
        X_of = [X[r].contiguous() for r in rows_of]
        eng = DemuxEngine(X[:4].cpu().numpy(), window, penalty)
        centres = eng.medoids(X, lab, G, window=window, penalty=penalty).refs
        centres_host = centres.cpu().numpy()

        def band():
            eng.ctx.set_option(_lib.OPT_DBA_GENERAL, 0)
            return eng.dba_step(X, lab, centres, G, window=window, penalty=penalty, want_cost=True, want_runs=True)

        def general():
            eng.ctx.set_option(_lib.OPT_DBA_GENERAL, 1)
            try:
                return eng.dba_step(X, lab, centres, G, window=window, penalty=penalty, want_cost=True, want_runs=True)
            finally:
                eng.ctx.set_option(_lib.OPT_DBA_GENERAL, 0)

        def distance():
            eng.set_refs(centres_host, window, penalty)
            return [eng.dtw(X_of[g], want_argmin=False)[0] for g in range(G)]

        routes = (("band", band), ("general", general), ("distance", distance))
        last = {}
        for name, fn in routes:   # warm-up: buffers sized, kernels loaded
            last[name] = timed(fn)[1]
        ms = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, fn in routes:
                t, last[name] = timed(fn)
                ms[name].append(t)
        same = all(torch.equal(getattr(last["band"], k).view(torch.int32), getattr(last["general"], k).view(torch.int32))
                   for k in ("centres", "count", "inertia", "cost", "runs"))
        rooted = all(torch.equal(last["band"].cost[rows_of[g]].sqrt().to(torch.float32), last["distance"][g][:, g]) for g in range(G))
        rec = dict(L=L, window=window, penalty=penalty, labels=G, rows_per_label=m, band_equals_general_bitwise=same,
                   rooted_cost_equals_distance=rooted, routes={name: stats(ms[name]) for name, _ in routes})
        rec["band_over_distance"] = round(rec["routes"]["band"]["median_ms"] / rec["routes"]["distance"]["median_ms"], 3)
        rec["general_over_distance"] = round(rec["routes"]["general"]["median_ms"] / rec["routes"]["distance"]["median_ms"], 3)
        if first is None:   # the full run: 10 steps from the medoids (the medoid call included)
            run = lambda: eng.barycenters(X, lab, G, window=window, penalty=penalty, n_iter=10)
            timed(run)
            t = []
            for _ in range(max(3, args.reps // 2)):
                ms_run, out = timed(run)
                t.append(ms_run)
            hist = out[2].cpu().numpy()
            rec["barycenters_10_steps"] = dict(stats(t), steps=int(hist.shape[0]), inertia_first=float(hist[0].sum()),
                                               inertia_last=float(hist[-1].sum()))
            first = rec
        print(json.dumps(rec), flush=True)
        results.append(rec)
        eng.close()
        del X, X_of
        torch.cuda.empty_cache()

    # accuracy: barycenters against medoids as the reference set, on held-out rows of the same labels
    G, m, L, window, penalty = 10, 400, 110, 15, 0.1
    if args.max_rows:
        m = min(m, args.max_rows)
    X, lab, gen, truth = make(G, 2 * m, L, 1.0, 77)
    train = np.arange(len(lab)) % 2 == 0
    ti, hi = torch.from_numpy(np.flatnonzero(train)).to(dev), torch.from_numpy(np.flatnonzero(~train)).to(dev)
    eng = DemuxEngine(X[:4].cpu().numpy(), window, penalty)
    med = eng.medoids(X[ti].contiguous(), lab[train], G, window=window, penalty=penalty).refs
    bary, _, hist = eng.barycenters(X[ti].contiguous(), lab[train], G, window=window, penalty=penalty, n_iter=10)
    err = {}
    for name, refs in (("medoids", med), ("barycenters", bary)):
        eng.set_refs(refs, window, penalty)
        call = eng.nearest(X[hi].contiguous()).call.cpu().numpy()
        err[name] = float((call != lab[~train]).mean())
    eng.close()
    accuracy = dict(labels=G, train_rows=int(train.sum()), held_out_rows=int((~train).sum()), L=L, window=window, penalty=penalty, noise_sigma=1.0,
                    steps=int(hist.shape[0]), error_rate=err)
    print(json.dumps(accuracy), flush=True)
    doc = dict(tool="tools/bench_dba.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               clocks="as found: nothing set; every route warmed up once before the timed alternation",
               shapes=results, accuracy=accuracy)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
