"""Fpt_Boost tail: the boost kernel alone, and the tRNA flow in one call with and without it.

    python tools/bench_boost.py [--out profiles/NAME.json] [--parent-tree DIR] [--rows N] [--reads N]
    python tools/bench_boost.py --sweep [--out profiles/NAME.json] [--launches N]

The sizes of the shipped tRNA models are not known here (their files are not available), so two ASSUMED sizes stand in:
CatBoost's defaults (1 000 trees, depth 6, 4 classes) and a small model (100 trees, depth 4, 4 classes), both over the 25
features of the tRNA fingerprint, with random borders / leaves (the timing depends on their values only through which
leaves are gathered).
  kernel   wdx_boost_predict_dev on --rows device-resident N(0, 1) fingerprints: reads/s, the kernel's HIP-event time
           (WDX_K_BOOST) and the achieved bytes/s of the leaf gathers (rows * trees * dim * 8 bytes over that time);
  flow     the tRNA flow (120 events, d = 9, W = 18, consensus refinement, K = 25) on --reads synthetic reads, in one session:
           (a) `demux_refine` of the parent commit, in a child process against --parent-tree (a checkout of the parent with
               its library built), on the same seeded reads -- the baseline;
           (b) `demux_refine` of this tree;
           (c) `demux_boost` with each model: reads/s, WDX_K_BOOST per call and its share of fingerprint + boost kernel time.
  --sweep  the two boost kernels against each other on minibatch-sized batches (WDX_OPT_BOOST_KERNEL): the
           HIP-event time of ONE wdx_boost_predict_dev launch for n in SWEEP_N and both models, options 1 (lane per read, the
           baseline) and 2 (tree-parallel) alternated in one process, every shape warmed up, --launches launches per point
           and pass, two passes per kernel; the spread of a point is the larger of the two kernels' differences between
           their passes' medians.  `n_small` = the largest swept n up to which, for BOTH models, the tree-parallel median
           beats the baseline's by more than that spread (0 if it does not at n = 1000): the value
           WDX_BOOST_SMALL_MAX_READS is set from.
The alternative a user had before -- fingerprints to the host and CatBoost with thread_count=1 -- is NOT measured: CatBoost is
not installed here.  One JSON document on stdout (and in --out).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"default_1000x6x4": (1000, 6, 4), "small_100x4x4": (100, 4, 4)}
K_FPT = 25
SEG = dict(min_obs_per_base=9, running_stat_width=18, num_events=120)


def _reads(n, seed=3):
    """n reads that carry the consensus between a random lead and a 30-event barcode (as tools/bench_refine.py)"""
    consensus = np.load(os.path.join(ROOT, "tests", "golden", "g8_refine.npz"))["consensus"]
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        lv = np.concatenate([rng.normal(0, 1, int(rng.integers(2, 34))), consensus, rng.normal(0, 1, 30)]) * 12.0 + 85.0
        dw = rng.integers(12, 40, lv.size)
        rows.append((np.repeat(lv, dw) + rng.normal(0, 1.5, int(dw.sum()))).astype(np.float32))
    stride = max(r.size for r in rows)
    mb = np.full((n, stride), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        mb[i, : r.size] = r
    return mb, np.full(n, 100, dtype=np.int32), np.array([r.size - 100 for r in rows], dtype=np.int32), consensus


def _engine_and_reads(n):
    import torch

    from warpdemux_amd import sig_proc
    from warpdemux_amd.engine import DemuxEngine

    mb, a_s, a_e, consensus = _reads(n)
    eng = DemuxEngine(np.zeros((1, K_FPT)), 15, 0.1, sig_proc.SegParams(barcode_num_events=K_FPT, **SEG))
    ref = sig_proc.RefineParams(query=consensus, barcode_segm_events=K_FPT, barcode_keep_events=K_FPT)
    d = lambda a: torch.from_numpy(a).to(eng.tdev)   # noqa: E731
    return eng, ref, d(mb), d(a_s), d(a_e), mb.shape[1]


def _timed(eng, fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    eng.kernel_timing(True)
    eng.kernel_time_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    return dt, out


def leg_demux_refine(n, reps):
    """`demux_refine` of whatever warpdemux_amd is first on sys.path (the parent tree in the child process)"""
    from warpdemux_amd import _lib

    eng, ref, sig, a_s, a_e, stride = _engine_and_reads(n)
    dt, out = _timed(eng, lambda: eng.demux_refine(sig, a_s, a_e, ref, stride=stride, max_len=stride), reps)
    r = dict(seconds=dt, reads_per_s=n / dt, fingerprint_ms=eng.kernel_time(_lib.K_FINGERPRINT)[0] / reps,
             ok_reads=int((out[0].status == 0).sum().item()))
    eng.close()
    return r


def _model(name, seed=0):
    from warpdemux_amd import models

    n_trees, depth, dim = MODELS[name]
    rng = np.random.default_rng(seed)
    trees = [(rng.integers(0, K_FPT, depth), rng.uniform(-1.5, 1.5, depth).astype(np.float32), np.zeros(depth, np.uint8),
              rng.normal(0, 2 / np.sqrt(n_trees), (1 << depth, dim))) for _ in range(n_trees)]
    return models.Fpt_Boost(trees, K_FPT, 1.0, rng.normal(0, 0.5, dim), {i: i for i in range(dim)})


def leg_kernel(rows, reps):
    import torch

    from warpdemux_amd import _lib

    eng, *_ = _engine_and_reads(8)
    X = torch.randn((rows, K_FPT), dtype=torch.float64, device=eng.tdev, generator=torch.Generator(eng.tdev).manual_seed(1))
    out = {}
    for name, (n_trees, depth, dim) in MODELS.items():
        eng.set_boost(_model(name))
        dt, res = _timed(eng, lambda: eng.boost_predict(X), reps)
        ms = eng.kernel_time(_lib.K_BOOST)[0] / reps
        out[name] = dict(rows=rows, seconds=dt, reads_per_s=rows / dt, boost_kernel_ms=ms,
                         kernel_reads_per_s=rows / (ms * 1e-3) if ms else None,
                         leaf_gather_bytes=rows * n_trees * dim * 8,
                         leaf_gather_bytes_per_s=rows * n_trees * dim * 8 / (ms * 1e-3) if ms else None,
                         leaf_table_bytes=n_trees * (1 << depth) * dim * 8, pred_hist=torch.bincount(res[1].long() + 1).tolist())
    eng.close()
    return out


SWEEP_N = (64, 256, 512, 1000, 4096, 16384, 65536)


def leg_sweep(launches):
    import torch

    from warpdemux_amd import _lib

    eng, *_ = _engine_and_reads(8)
    gen = torch.Generator(eng.tdev).manual_seed(1)
    X = torch.randn((max(SWEEP_N), K_FPT), dtype=torch.float64, device=eng.tdev, generator=gen)
    names = {1: "lane_per_read", 2: "tree_parallel"}

    def point(option, x):
        """per-launch HIP-event times (ms) of `launches` launches"""
        eng.ctx.set_option(_lib.OPT_BOOST_KERNEL, option)
        ms = []
        for _ in range(launches):
            eng.kernel_time_reset()
            eng.boost_predict(x)
            ms.append(eng.kernel_time(_lib.K_BOOST)[0])
        return ms

    out, wins = {}, {}
    eng.kernel_timing(True)
    try:
        for name in MODELS:
            eng.set_boost(_model(name))
            table = {}
            for n in SWEEP_N:
                x = X[:n].contiguous()
                same = True
                for option in (1, 2):   # warm-up of the shape under both kernels, and the two must agree
                    eng.ctx.set_option(_lib.OPT_BOOST_KERNEL, option)
                    res = [t.clone() for t in eng.boost_predict(x, want_raw=True)]
                    for _ in range(10):
                        eng.boost_predict(x)
                    if option == 1:
                        first = res
                    else:
                        same = all(torch.equal(a, b) for a, b in zip(first, res))
                torch.cuda.synchronize()
                passes = {1: [], 2: []}
                for _ in range(2):
                    for option in (1, 2):
                        passes[option].append(point(option, x))
                row = dict(bit_identical=bool(same))
                for option in (1, 2):
                    meds = [float(np.median(p)) for p in passes[option]]
                    row[names[option]] = dict(median_ms=float(np.median(np.concatenate(passes[option]))), pass_medians_ms=meds,
                                              spread_ms=abs(meds[0] - meds[1]), min_ms=float(np.min(passes[option])))
                spread = max(row[names[1]]["spread_ms"], row[names[2]]["spread_ms"])
                gain = row[names[1]]["median_ms"] - row[names[2]]["median_ms"]
                row.update(spread_ms=spread, gain_ms=gain, tree_parallel_wins=bool(gain > spread),
                           speedup=row[names[1]]["median_ms"] / row[names[2]]["median_ms"])
                table[str(n)] = row
                wins.setdefault(n, []).append(row["tree_parallel_wins"])
            out[name] = table
    finally:
        eng.ctx.set_option(_lib.OPT_BOOST_KERNEL, 0)
        eng.close()
    n_small = 0
    if all(wins[1000]):
        for n in SWEEP_N:
            if not all(wins[n]):
                break
            n_small = n
    return dict(launches_per_point_and_pass=launches, passes=2, sweep=out, n_small=n_small,
                built_with_small_max_reads=_lib.BOOST_SMALL_MAX_READS)


def leg_flow(n, reps):
    from warpdemux_amd import _lib

    eng, ref, sig, a_s, a_e, stride = _engine_and_reads(n)
    out = {}
    for name in MODELS:
        eng.set_boost(_model(name))
        dt, res = _timed(eng, lambda: eng.demux_boost(sig, a_s, a_e, ref, stride=stride, max_len=stride), reps)
        fp_ms, boost_ms = eng.kernel_time(_lib.K_FINGERPRINT)[0] / reps, eng.kernel_time(_lib.K_BOOST)[0] / reps
        out[name] = dict(seconds=dt, reads_per_s=n / dt, fingerprint_ms=fp_ms, boost_kernel_ms=boost_ms,
                         boost_share_of_kernel_time=boost_ms / (fp_ms + boost_ms) if fp_ms + boost_ms else None,
                         ok_reads=int((res[3] == 0).sum().item()))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--parent-tree", help="checkout of the parent commit with its library built (leg a)")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--leg-a", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--sweep", action="store_true", help="the two boost kernels on minibatch-sized batches (see above)")
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    if args.leg_a:   # child process: sys.path[0] is the parent tree
        print(json.dumps(leg_demux_refine(args.reads, args.reps)))
        return
    sys.path.insert(0, ROOT)
    if args.sweep:
        doc = dict(assumption="model sizes are assumed (CatBoost defaults and a small model)", n_features=K_FPT,
                   **leg_sweep(args.launches))
        text = json.dumps(doc, indent=1)
        print(text)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(text + "\n")
        return
    doc = dict(assumption="model sizes are assumed (CatBoost defaults and a small model): the shipped tRNA models' sizes are "
                          "unknown; parity with CatBoost is unpinned and the host CatBoost path is not measured",
               n_features=K_FPT, reps=args.reps)
    if args.parent_tree:
        env = dict(os.environ, PYTHONPATH=os.path.abspath(args.parent_tree))
        env.pop("WDX_LIB_PATH", None)
        cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg-a", "--reads", str(args.reads), "--reps",
                             str(args.reps)], env=env, cwd=args.parent_tree, capture_output=True, text=True, check=True)
        doc["flow_parent_demux_refine"] = json.loads(cp.stdout.strip().splitlines()[-1])
    doc["flow_demux_refine"] = leg_demux_refine(args.reads, args.reps)
    doc["flow_demux_boost"] = leg_flow(args.reads, args.reps)
    doc["kernel"] = leg_kernel(args.rows, args.reps)
    doc["reads"] = args.reads
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
