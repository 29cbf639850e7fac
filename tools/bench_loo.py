#!/usr/bin/env python3
"""What the leave-one-out nearest neighbours of a labelled set cost on one MI355X, alternating in one process:

  loo          `DemuxEngine.loo_nearest` as shipped: the self matrix's tile walk with the nearest rule as its epilogue, partial
               results merged as 64-bit keys by an atomic minimum, no (n, n) matrix (wdx_dtw_loo.hip)
  loo_general  the same call with WDX_OPT_SELF_NEAREST_GENERAL = 1: row blocks of at most 96 MiB through the DTW dispatch, then the
               rows kernel (16 384 rows only)
  self         `DemuxEngine.self_distances` alone on the same rows, into a matrix allocated beforehand: the DTW work of the parent
               route without its reduction
  parent       what a user could do before this entry existed: `self_distances`, then the masked row minima in torch (own label
               without the diagonal, other labels), in row blocks of 4 096 rows; its peak device memory is recorded

Workloads: n = 16 384 (median of --reps alternations behind a warm-up) and 65 536 (--big-reps), L 110, window 15, penalty 0.1, 10
labels.  Every call is bracketed by device events and followed by a synchronise; per route: median / min / max ms and the spread
(max - min) / median.  Before anything is timed, nn and best of `loo` are verified against the parent route's reduction done
exactly (the rule's 64-bit keys built from the self matrix in torch), and `loo_general` against `loo`, bit for bit.

The breakdown (--no-split skips it): the same calls in a child process under `rocprofv3 --kernel-trace --stats`, from whose
per-kernel statistics come the finish kernel's time, the time of the pre-pass and the finish pass together as a share of the call
(the merge's passes), and the tile kernels' time next to the self matrix's tile kernels (what the reduction and the atomic
minima cost against the two images they replace: the atomics themselves cannot be separated from the kernel they run in).

    python tools/bench_loo.py --out profiles/loo_nearest.json
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

L, WINDOW, PENALTY, N_LABELS = 110, 15, 0.1, 10
SIZES = [16384]
BIG = 65536
PARENT_BLOCK = 4096
# -Rpass-analysis=kernel-resource-usage of wdx_dtw_loo.hip (gfx950): VGPRs, scratch bytes / lane, LDS bytes / wave, waves / SIMD
# (self_tile_kernel<15 exact>: 164 / 0 / 8 320 / 3 off the diagonal, 149 / 0 / 16 640 / 3 on it)
KERNEL_RESOURCES = {
    "loo_tile_kernel<15 exact, off-diagonal>": dict(vgprs=158, scratch=0, lds=10880, waves_per_simd=3),
    "loo_tile_kernel<15 exact, diagonal>": dict(vgprs=166, scratch=0, lds=16896, waves_per_simd=3),
}


def make_rows(torch, n, dev):
    gen = torch.Generator(device=dev).manual_seed(1000 * L + n % 997)
    centres = torch.randn((N_LABELS, L), generator=gen, device=dev, dtype=torch.float64).cumsum(dim=1) * 0.3
    labels = torch.randint(0, N_LABELS, (n,), generator=gen, device=dev, dtype=torch.int32)
    X = (centres[labels.long()] + 0.35 * torch.randn((n, L), generator=gen, device=dev, dtype=torch.float64)).contiguous()
    return X, labels


def parent_reduce(torch, D, labels):
    """the masked row minima a user would take of the self matrix: (nn (n, 2) int64, best (n, 2) float32)"""
    n = D.shape[0]
    nn = torch.empty((n, 2), dtype=torch.int64, device=D.device)
    best = torch.empty((n, 2), dtype=torch.float32, device=D.device)
    inf = float("inf")
    for r0 in range(0, n, PARENT_BLOCK):
        blk = D[r0:r0 + PARENT_BLOCK]
        same = labels[r0:r0 + PARENT_BLOCK, None] == labels[None, :]
        rows = torch.arange(r0, r0 + blk.shape[0], device=D.device)
        own = blk.masked_fill(~same, inf)
        own[torch.arange(blk.shape[0], device=D.device), rows] = inf
        best[r0:r0 + PARENT_BLOCK, 0], nn[r0:r0 + PARENT_BLOCK, 0] = own.min(dim=1)
        best[r0:r0 + PARENT_BLOCK, 1], nn[r0:r0 + PARENT_BLOCK, 1] = blk.masked_fill(same, inf).min(dim=1)
    return nn, best


def exact_reduce(torch, D, labels):
    """the rule itself on the self matrix (every row a member here): the minimum of (float32 bits << 32 | column) per side"""
    n = D.shape[0]
    nn = torch.empty((n, 2), dtype=torch.int32, device=D.device)
    best = torch.empty((n, 2), dtype=torch.float32, device=D.device)
    cols = torch.arange(n, device=D.device, dtype=torch.int64)
    none = torch.iinfo(torch.int64).max
    for r0 in range(0, n, 2048):
        blk = D[r0:r0 + 2048]
        keys = (blk.view(torch.int32).to(torch.int64) << 32) | cols[None, :]
        same = labels[r0:r0 + 2048, None] == labels[None, :]
        diag = cols[None, :] == (cols[r0:r0 + blk.shape[0], None])
        for side, mask in enumerate((same & ~diag, ~same)):
            k = keys.masked_fill(~mask, none).min(dim=1).values
            nn[r0:r0 + 2048, side] = torch.where(k == none, -1, k & 0xFFFFFFFF).to(torch.int32)
            best[r0:r0 + 2048, side] = torch.where(k == none, 0x7F800000, k >> 32).to(torch.int32).view(torch.float32)
    return nn, best


def child(n, reps):
    """what runs under the profiler: `reps` warm calls of loo_nearest and of self_distances"""
    import torch

    from warpdemux_amd.engine import DemuxEngine

    dev = torch.device("cuda", 0)
    X, labels = make_rows(torch, n, dev)
    eng = DemuxEngine(X[:4].cpu().numpy(), WINDOW, PENALTY)
    D = torch.empty((n, n), dtype=torch.float32, device=dev)
    for _ in range(reps + 1):
        eng.loo_nearest(X, labels, window=WINDOW, penalty=PENALTY)
        eng.self_distances(X, WINDOW, PENALTY, out=D)
    torch.cuda.synchronize()
    eng.close()


def kernel_split(n, reps):
    """per-kernel statistics of `child` under rocprofv3 --kernel-trace --stats -> the breakdown (or the reason there is none)"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", str(n), "--reps", str(reps)]
        try:
            run = subprocess.run(cmd, capture_output=True, timeout=600, cwd=d)
        except (OSError, subprocess.TimeoutExpired) as e:
            return dict(error=repr(e))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if run.returncode != 0 or not files:
            return dict(error="rocprofv3 exit %d, %d statistics files: %s" % (run.returncode, len(files), run.stderr.decode()[-400:]))
        stats = {}
        for f in files:
            for row in csv.DictReader(open(f)):
                name = row.get("Name", "")
                m = re.search(r"(loo_tile_kernel|self_tile_kernel)<([^>]*)>", name)
                if m:
                    key = "%s<%s>" % (m.group(1), "diag" if m.group(2).replace(" ", "").endswith("true") else "off")
                else:
                    m = re.search(r"(loo_[a-z_]+_kernel|tile_gather_kernel)", name)
                    if not m:
                        continue
                    key = m.group(1)
                s = stats.setdefault(key, dict(calls=0, total_ns=0))
                s["calls"] += int(row["Calls"])
                s["total_ns"] += int(float(row["TotalDurationNs"]))
    calls = reps + 1
    per_call = {k: round(v["total_ns"] / calls * 1e-6, 4) for k, v in stats.items()}   # ms per API call
    out = dict(n=n, calls=calls, ms_per_call=per_call, raw=stats)
    loo_tiles = per_call.get("loo_tile_kernel<diag>", 0) + per_call.get("loo_tile_kernel<off>", 0)
    self_tiles = per_call.get("self_tile_kernel<diag>", 0) + per_call.get("self_tile_kernel<off>", 0)
    finish, init = per_call.get("loo_finish_kernel"), per_call.get("loo_init_kernel")
    if finish is not None and init is not None and loo_tiles:
        gather = per_call.get("tile_gather_kernel", 0) / 2.0    # (both entries launch it once per call)
        total = loo_tiles + finish + init + gather
        out.update(finish_kernel_ms=finish, init_kernel_ms=init, loo_tile_kernels_ms=round(loo_tiles, 4), self_tile_kernels_ms=round(self_tiles, 4),
                   merge_passes_share_of_call=round((finish + init) / total, 6),
                   tile_kernels_loo_over_self=round(loo_tiles / self_tiles, 4) if self_tiles else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="alternations after the warm-up")
    ap.add_argument("--big-reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--big", type=int, default=BIG, help="the large size (0: none)")
    ap.add_argument("--no-split", action="store_true", help="no child process under rocprofv3")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps)

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
    for n, reps in [(n, args.reps) for n in args.sizes] + ([(args.big, args.big_reps)] if args.big else []):
        X, labels = make_rows(torch, n, dev)
        eng = DemuxEngine(X[:4].cpu().numpy(), WINDOW, PENALTY)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        res = eng.loo_nearest(X, labels, window=WINDOW, penalty=PENALTY)
        torch.cuda.synchronize()
        loo_device_bytes = free0 - torch.cuda.mem_get_info()[0]     # the context's workspace and the two outputs
        # -- verify before anything is timed
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        D = eng.self_distances(X, WINDOW, PENALTY)
        p_nn, p_best = parent_reduce(torch, D, labels)
        torch.cuda.synchronize()
        parent_peak = torch.cuda.max_memory_allocated() - base
        w_nn, w_best = exact_reduce(torch, D, labels)
        verified = dict(nn_equals_rule_on_self_matrix=bool(torch.equal(res.nn, w_nn)),
                        best_equals_rule_on_self_matrix_bitwise=bool(torch.equal(res.best.view(torch.int32), w_best.view(torch.int32))),
                        best_equals_torch_minima_bitwise=bool(torch.equal(res.best.view(torch.int32), p_best.view(torch.int32))),
                        nn_differs_from_torch_minima=int((res.nn.long() != p_nn).sum()))
        if not (verified["nn_equals_rule_on_self_matrix"] and verified["best_equals_rule_on_self_matrix_bitwise"]):
            raise SystemExit("loo_nearest differs from the rule on the self matrix at n = %d: %r" % (n, verified))
        del p_nn, p_best, w_nn, w_best

        def loo():
            return eng.loo_nearest(X, labels, window=WINDOW, penalty=PENALTY)

        def loo_general():
            eng.ctx.set_option(_lib.OPT_SELF_NEAREST_GENERAL, 1)
            try:
                return eng.loo_nearest(X, labels, window=WINDOW, penalty=PENALTY)
            finally:
                eng.ctx.set_option(_lib.OPT_SELF_NEAREST_GENERAL, 0)

        def self_only():
            return eng.self_distances(X, WINDOW, PENALTY, out=D)

        def parent():
            return parent_reduce(torch, eng.self_distances(X, WINDOW, PENALTY, out=D), labels)

        routes = [("loo", loo)] + ([("loo_general", loo_general)] if n <= 16384 else []) + [("self", self_only), ("parent", parent)]
        if len(routes) == 4:
            g = loo_general()
            verified["general_equals_tile_bitwise"] = bool(torch.equal(g.nn, res.nn) and torch.equal(g.best.view(torch.int32), res.best.view(torch.int32)))
        for _, fn in routes:   # warm-up
            timed(fn)
        ms = {name: [] for name, _ in routes}
        for _ in range(reps):
            for name, fn in routes:
                ms[name].append(timed(fn)[0])
        rec = dict(L=L, window=WINDOW, penalty=PENALTY, n=n, n_labels=N_LABELS, reps=reps, verified=verified, matrix_bytes=4 * n * n,
                   parent_peak_device_bytes=int(parent_peak), loo_device_bytes_first_call=int(loo_device_bytes),
                   loo_device_bytes_over_n_L_8=round(loo_device_bytes / (n * L * 8.0), 3), routes={})
        for name, _ in routes:
            med = statistics.median(ms[name])
            rec["routes"][name] = dict(median_ms=round(med, 3), min_ms=round(min(ms[name]), 3), max_ms=round(max(ms[name]), 3),
                                       spread=round((max(ms[name]) - min(ms[name])) / med, 4))
        r = rec["routes"]
        rec["loo_over_self"] = round(r["loo"]["median_ms"] / r["self"]["median_ms"], 4)
        rec["parent_over_loo"] = round(r["parent"]["median_ms"] / r["loo"]["median_ms"], 4)
        rec["loo_no_longer_than_self_beyond_spread"] = bool(r["loo"]["median_ms"] <= r["self"]["median_ms"] * (1 + max(r["loo"]["spread"], r["self"]["spread"])))
        print(json.dumps(rec), flush=True)
        results.append(rec)
        eng.close()
        del X, labels, D, res
        torch.cuda.empty_cache()
    split = None
    if not args.no_split:
        split = kernel_split(args.sizes[0] if args.sizes else args.big, 3)
        print(json.dumps(dict(kernel_split=split)), flush=True)
    doc = dict(tool="tools/bench_loo.py", device=torch.cuda.get_device_name(0), kernel_resources=KERNEL_RESOURCES, shapes=results, kernel_split=split)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
