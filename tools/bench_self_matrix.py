#!/usr/bin/env python3
"""What the (n, n) DTW self-distance matrix -- the training matrix of a DTW_SVM -- costs on one MI355X, alternating in one process:

  tile         `DemuxEngine.self_distances` as shipped: one wave per 64 x 64 tile, each unordered pair once, both images written
               (wdx_dtw_self.hip)
  tile_band15  (L 25 only) the same with WDX_OPT_NO_SHORT_DTW = 1: the band-15 tile kernel in place of the unrolled 25-point one
  general      the same call with WDX_OPT_SELF_MATRIX_GENERAL = 1: row blocks through the DTW dispatch, then the mask kernel
  parent       what a user could do before this entry existed: `set_refs(X)`, then `DemuxEngine.dtw` in row blocks of 2 048 rows
               writing into the same (n, n) matrix -- every unordered pair twice; the yardstick

Shapes: n = 4 096 and 16 384 (median of --reps alternations), and 65 536 once (--big), each at (L 110, window 15, penalty 0.1) and
(25, 15, 0.1).  Every call is bracketed by device events and followed by a synchronise; per route: median / min / max ms, the
spread (max - min) / median, and USEFUL cell updates per second -- unordered pairs (the diagonal included) x cells inside the band
/ median, whatever the route really computed -- next to the medoid path's measured rate (profiles/medoids.json), which this
kernel's work exceeds by 2 x 16 KiB of stores per tile.  All routes are compared bit for bit at the timed size.

    python tools/bench_self_matrix.py --out profiles/self_matrix.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [4096, 16384]
BIG = 65536
PARAMS = [(110, 15, 0.1), (25, 15, 0.1)]
PARENT_BLOCK = 2048
# -Rpass-analysis=kernel-resource-usage of wdx_dtw_self.hip (gfx950): VGPRs, scratch bytes / lane, LDS bytes / wave, waves / SIMD
KERNEL_RESOURCES = {
    "self_tile_kernel<15 exact, off-diagonal>": dict(vgprs=164, scratch=0, lds=8320, waves_per_simd=3),
    "self_tile_kernel<15 exact, diagonal>": dict(vgprs=149, scratch=0, lds=16640, waves_per_simd=3),
    "self_tile_kernel<short 25/15, off-diagonal>": dict(vgprs=168, scratch=180, lds=8320, waves_per_simd=3),
    "self_tile_kernel<short 25/15, diagonal>": dict(vgprs=164, scratch=0, lds=16640, waves_per_simd=3),
    "self_tile_kernel<8, off-diagonal>": dict(vgprs=72, scratch=0, lds=8320, waves_per_simd=5),
    "self_tile_kernel<16, off-diagonal>": dict(vgprs=104, scratch=0, lds=8320, waves_per_simd=4),
    "self_tile_kernel<32, off-diagonal>": dict(vgprs=168, scratch=0, lds=8320, waves_per_simd=3),
}


def band_cells(L, w):
    w = L if (w is None or w <= 0 or w > L) else w
    return L * L - (L - w) * (L - w + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="alternations after the warm-up")
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--big", type=int, default=BIG, help="the size measured once, without a warm-up of its own (0: none)")
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
        for n, reps in [(n, args.reps) for n in args.sizes] + ([(args.big, 1)] if args.big else []):
            gen = torch.Generator(device=dev).manual_seed(1000 * L + n % 997)
            centres = torch.randn((8, L), generator=gen, device=dev, dtype=torch.float64).cumsum(dim=1) * 0.3
            pick = torch.randint(0, 8, (n,), generator=gen, device=dev)
            X = (centres[pick] + 0.35 * torch.randn((n, L), generator=gen, device=dev, dtype=torch.float64)).contiguous()
            Xh = X.cpu().numpy()
            eng = DemuxEngine(Xh[:4], window, penalty)
            out = {}

            def buffer(name):
                if name not in out:
                    out[name] = torch.empty((n, n), dtype=torch.float32, device=dev)
                return out[name]

            def with_option(opt, name):
                eng.ctx.set_option(opt, 1)
                try:
                    return eng.self_distances(X, window, penalty, out=buffer(name))
                finally:
                    eng.ctx.set_option(opt, 0)

            def tile():
                return eng.self_distances(X, window, penalty, out=buffer("tile"))

            def tile_band15():
                return with_option(_lib.OPT_NO_SHORT_DTW, "tile_band15")

            def general():
                return with_option(_lib.OPT_SELF_MATRIX_GENERAL, "general")

            def parent():
                D = buffer("parent")
                eng.set_refs(Xh, window, penalty)
                for r0 in range(0, n, PARENT_BLOCK):
                    eng.dtw(X[r0:r0 + PARENT_BLOCK], want_argmin=False, out=(D[r0:r0 + PARENT_BLOCK], None))
                return D

            routes = [("tile", tile)] + ([("tile_band15", tile_band15)] if L == 25 else []) + [("general", general), ("parent", parent)]
            last = {}
            if reps > 1:
                for name, fn in routes:   # warm-up: buffers sized, kernels loaded
                    last[name] = timed(fn)[1]
            ms = {name: [] for name, _ in routes}
            for _ in range(reps):
                for name, fn in routes:
                    t, last[name] = timed(fn)
                    ms[name].append(t)
            same = {name: bool(torch.equal(last[name].view(torch.int32), last["tile"].view(torch.int32))) for name, _ in routes[1:]}
            pairs = n * (n + 1) // 2
            useful = pairs * band_cells(L, window)
            rec = dict(L=L, window=window, penalty=penalty, n=n, reps=reps, warm=reps > 1, unordered_pairs=pairs, useful_cell_updates=useful,
                       matrix_bytes=4 * n * n, equals_tile_bitwise=same, routes={})
            for name, _ in routes:
                med = statistics.median(ms[name])
                rec["routes"][name] = dict(median_ms=round(med, 3), min_ms=round(min(ms[name]), 3), max_ms=round(max(ms[name]), 3),
                                           spread=round((max(ms[name]) - min(ms[name])) / med, 4),
                                           useful_cell_updates_per_s=round(useful / (med * 1e-3), 1))
            for name, _ in routes[:-1]:
                rec[name + "_speedup_over_parent"] = round(rec["routes"]["parent"]["median_ms"] / rec["routes"][name]["median_ms"], 3)
            print(json.dumps(rec), flush=True)
            results.append(rec)
            eng.close()
            del X, out, last
            torch.cuda.empty_cache()
    doc = dict(tool="tools/bench_self_matrix.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               medoid_path_cell_updates_per_s="profiles/medoids.json: 6.32e12 (1 x 16 384, L 110), 4.87e12 (1 x 16 384, L 25)",
               kernel_resources=KERNEL_RESOURCES, shapes=results)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
