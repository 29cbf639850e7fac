#!/usr/bin/env python3
"""What per-label DTW medoids cost on one MI355X, three ways, alternating in one process:

  tile      `DemuxEngine.medoids` as shipped: one wave per 64 x 64 tile, each unordered pair once (wdx_medoid.hip)
  general   the same call with WDX_OPT_MEDOID_GENERAL = 1: the label's matrix block by block through the DTW dispatch, chunk sums
  parent    what a user could do before this entry existed, label by label: `set_refs(X_g)`, `DemuxEngine.dtw` in row blocks of
            2 048 rows, a torch float64 row sum per block, argmin -- the yardstick

Shapes: one label of 16 384 rows, and 10 labels of 4 096 rows, each at (L 110, window 15, penalty 0.1) and (25, 15, 0.1).  Every
call is bracketed by device events and followed by a synchronise; per route: median / min / max ms over the repetitions, the
spread (max - min) / median, and USEFUL cell updates per second -- unordered pairs (the diagonal included) x cells inside the
band / median, whatever the route really computed -- next to the band kernel's published 6.4-6.5 T/s (README).  tile and general
are compared bit for bit at the timed size; the parent route's medoids are compared by index (its sums run in another order).

    python tools/bench_medoids.py --out profiles/medoids.json
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

# (labels, rows per label)
GROUPS = [(1, 16384), (10, 4096)]
PARAMS = [(110, 15, 0.1), (25, 15, 0.1)]
PARENT_BLOCK = 2048
# -Rpass-analysis=kernel-resource-usage of wdx_medoid.hip (gfx950): VGPRs, spilled VGPRs, scratch bytes / lane, LDS bytes / wave,
# waves / SIMD by registers; twelve waves of the off-diagonal kernels' 8 320 B of LDS are 97.5 KiB of a CU's 160 KiB
KERNEL_RESOURCES = {
    "medoid_tile_kernel<15 exact, off-diagonal>": dict(vgprs=168, vgpr_spill=0, scratch=0, lds=8320, waves_per_simd=3),
    "medoid_tile_kernel<15 exact, diagonal>": dict(vgprs=146, vgpr_spill=0, scratch=0, lds=16640, waves_per_simd=3),
    "medoid_tile_kernel<short 25/15, off-diagonal>": dict(vgprs=168, vgpr_spill=19, scratch=80, lds=8320, waves_per_simd=3),
    "medoid_tile_kernel<short 25/15, diagonal>": dict(vgprs=162, vgpr_spill=0, scratch=0, lds=16640, waves_per_simd=3),
    "medoid_tile_kernel<8, off-diagonal>": dict(vgprs=62, vgpr_spill=0, scratch=0, lds=8320, waves_per_simd=8),
    "medoid_tile_kernel<16, off-diagonal>": dict(vgprs=94, vgpr_spill=0, scratch=0, lds=8320, waves_per_simd=5),
    "medoid_tile_kernel<32, off-diagonal>": dict(vgprs=158, vgpr_spill=0, scratch=0, lds=8320, waves_per_simd=3),
}


def band_cells(L, w):
    w = L if (w is None or w <= 0 or w > L) else w
    return L * L - (L - w) * (L - w + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="alternations after the warm-up")
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

    results = []
    for L, window, penalty in PARAMS:
        for G, m in GROUPS:
            if args.max_rows:
                m = min(m, args.max_rows)
            n = G * m
            gen = torch.Generator(device=dev).manual_seed(1000 * L + G)
            centres = torch.randn((G, L), generator=gen, device=dev, dtype=torch.float64).cumsum(dim=1) * 0.3
            lab = np.repeat(np.arange(G, dtype=np.int32), m)
            np.random.default_rng(G).shuffle(lab)
            X = (centres[torch.from_numpy(lab.astype(np.int64)).to(dev)] +
                 0.35 * torch.randn((n, L), generator=gen, device=dev, dtype=torch.float64)).contiguous()
            rows_of = [torch.from_numpy(np.flatnonzero(lab == g)).to(dev) for g in range(G)]
            eng = DemuxEngine(X[:4].cpu().numpy(), window, penalty)

            def tile():
                eng.ctx.set_option(_lib.OPT_MEDOID_GENERAL, 0)
                return eng.medoids(X, lab, G, window=window, penalty=penalty, want_cost=True)

            def general():
                eng.ctx.set_option(_lib.OPT_MEDOID_GENERAL, 1)
                try:
                    return eng.medoids(X, lab, G, window=window, penalty=penalty, want_cost=True)
                finally:
                    eng.ctx.set_option(_lib.OPT_MEDOID_GENERAL, 0)

            def parent():
                index = []
                for g in range(G):
                    Xg = X[rows_of[g]].contiguous()
                    eng.set_refs(Xg.cpu().numpy(), window, penalty)
                    cost = torch.empty(m, dtype=torch.float64, device=dev)
                    for r0 in range(0, m, PARENT_BLOCK):
                        dist, _ = eng.dtw(Xg[r0:r0 + PARENT_BLOCK], want_argmin=False)
                        cost[r0:r0 + PARENT_BLOCK] = dist.to(torch.float64).sum(dim=1)
                    index.append(rows_of[g][torch.argmin(cost)])
                return torch.stack(index)

            routes = (("tile", tile), ("general", general), ("parent", parent))
            last = {}
            for name, fn in routes:   # warm-up: buffers sized, kernels loaded
                last[name] = timed(fn)[1]
            ms = {name: [] for name, _ in routes}
            for _ in range(args.reps):
                for name, fn in routes:
                    t, last[name] = timed(fn)
                    ms[name].append(t)
            same = all(torch.equal(getattr(last["tile"], k).view(torch.int64), getattr(last["general"], k).view(torch.int64))
                       for k in ("index", "refs", "count", "medoid_cost", "cost"))
            parent_same = bool(torch.equal(last["parent"], last["tile"].index))
            useful = G * (m * (m + 1) // 2) * band_cells(L, window)
            rec = dict(L=L, window=window, penalty=penalty, labels=G, rows_per_label=m, unordered_pairs=G * (m * (m + 1) // 2),
                       useful_cell_updates=useful, tile_equals_general_bitwise=same, parent_medoids_equal=parent_same, routes={})
            for name, _ in routes:
                med = statistics.median(ms[name])
                rec["routes"][name] = dict(median_ms=round(med, 3), min_ms=round(min(ms[name]), 3), max_ms=round(max(ms[name]), 3),
                                           spread=round((max(ms[name]) - min(ms[name])) / med, 4),
                                           useful_cell_updates_per_s=round(useful / (med * 1e-3), 1))
            rec["tile_speedup_over_parent"] = round(rec["routes"]["parent"]["median_ms"] / rec["routes"]["tile"]["median_ms"], 3)
            rec["general_speedup_over_parent"] = round(rec["routes"]["parent"]["median_ms"] / rec["routes"]["general"]["median_ms"], 3)
            print(json.dumps(rec), flush=True)
            results.append(rec)
            eng.close()
            del X
            torch.cuda.empty_cache()
    doc = dict(tool="tools/bench_medoids.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               band_kernel_published_cell_updates_per_s="6.4e12 - 6.5e12 (README)", kernel_resources=KERNEL_RESOURCES, shapes=results)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
