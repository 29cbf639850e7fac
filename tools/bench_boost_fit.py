#!/usr/bin/env python3
"""What `Fpt_Boost.fit` costs on one MI355X, beside a host comparison on the same rows.

  device   `Fpt_Boost.fit` (wdx_boost_fit.hip): borders on the host, then 1 + trees x (3 depth + 4) launches with no synchronisation
           in between.  Recorded: the host borders pass, the whole call, the launches alone (the library's event pair,
           WDX_K_BOOST_FIT) and from them milliseconds per tree.
  split    the same fit with fewer trees in a child process under `rocprofv3 --kernel-trace --stats`: the share of every kernel of
           the trainer in the trainer's kernel time, and the histogram kernel's achieved bin visits per second
           (rows x features x depth per tree over its time; the extra pass over the final leaves is part of the time).
  sklearn  `HistGradientBoostingClassifier(max_iter=trees, max_depth=depth, max_bins=borders, learning_rate, l2_regularization,
           early_stopping=False)` on the OMP_NUM_THREADS host cores (16).  A DIFFERENT algorithm -- leaf-wise trees, one per class and
           iteration, float histograms -- so only the cost per boosting iteration and the held-out accuracy are comparable.
           `--host-trees` bounds its iterations (its time is reported per iteration).
  default  `--default-path`: the six reads/s of `python bench.py` alternated with the parent commit, recorded beside the figures.
  catboost wherever it imports: `CatBoostClassifier(iterations, depth, learning_rate, l2_leaf_reg, border_count, thread_count)`.

Shapes (CatBoost's defaults for trees, depth and borders -- an assumption): 30 000 x 25 x 4 classes,
200 000 x 25 x 4 and 200 000 x 120 x 10, each 1 000 trees of depth 6 on 128 borders.  Rows are class templates plus N(0, 1.5) noise.

    python tools/bench_boost_fit.py --out profiles/boost_fit.json
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"30k-25-4": (30000, 25, 4), "200k-25-4": (200000, 25, 4), "200k-120-10": (200000, 120, 10)}
N_TEST, LR, LAM = 4096, 0.3, 3.0


def make_rows(n, F, k, seed):
    rng = np.random.default_rng(seed)
    templates = rng.normal(0, 2.0, (k, F))
    y = rng.integers(0, k, n + N_TEST)
    X = templates[y] + rng.normal(0, 1.5, (n + N_TEST, F))
    return X[:n], y[:n], X[n:], y[n:]


def device_fit(Xtr, ytr, trees, depth, borders):
    from warpdemux_amd.models import Fpt_Boost

    return Fpt_Boost.fit(Xtr, ytr, n_trees=trees, depth=depth, learning_rate=LR, l2_leaf_reg=LAM, border_count=borders)


def child(shape, trees, depth, borders):
    n, F, k = SHAPES[shape]
    Xtr, ytr, _, _ = make_rows(n, F, k, 7)
    device_fit(Xtr, ytr, trees, depth, borders)


def kernel_split(shape, trees, depth, borders):
    """per-kernel statistics of `child` under rocprofv3 --kernel-trace --stats (or the reason there are none)"""
    n, F, _ = SHAPES[shape]
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", shape, "--trees", str(trees), "--depth", str(depth), "--borders", str(borders)]
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
                m = re.search(r"boost_fit_([a-z]+)_kernel", row.get("Name", ""))
                if m:
                    s = stats.setdefault(m.group(1), dict(calls=0, total_ns=0))
                    s["calls"] += int(row["Calls"])
                    s["total_ns"] += int(float(row["TotalDurationNs"]))
    total = sum(v["total_ns"] for v in stats.values())
    if not total or "hist" not in stats:
        return dict(error="no kernel of the trainer in the statistics")
    hist_s = stats["hist"]["total_ns"] * 1e-9
    return dict(trees=trees, kernels_ms_per_tree={k_: round(v["total_ns"] * 1e-6 / trees, 4) for k_, v in stats.items()},
                share={k_: round(v["total_ns"] / total, 4) for k_, v in stats.items()}, calls={k_: v["calls"] for k_, v in stats.items()},
                dominant=max(stats, key=lambda k_: stats[k_]["total_ns"]), hist_share=round(stats["hist"]["total_ns"] / total, 4),
                hist_bin_visits_per_s=float("%.4g" % (n * F * depth * trees / hist_s)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--borders", type=int, default=128)
    ap.add_argument("--host-trees", type=int, default=0, help="iterations of the host comparisons (0: as many as --trees)")
    ap.add_argument("--split-trees", type=int, default=50, help="trees of the fit under rocprofv3 (0: no child process)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--default-path", nargs=6, type=float, default=None, metavar="READS_PER_S",
                    help="record `python bench.py` alternated with the parent commit: this parent this parent this parent")
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.trees, args.depth, args.borders)

    import torch

    from warpdemux_amd import _boost_fit, _lib

    doc = dict(tool="tools/bench_boost_fit.py", device=torch.cuda.get_device_name(0), shapes=[])
    if args.out and os.path.exists(args.out):   # (shapes measured by an earlier call stay, and so does the bench.py alternation)
        old = json.load(open(args.out))
        doc["shapes"] = [s for s in old.get("shapes", []) if s["shape"] not in args.shapes]
        doc.update({k_: v for k_, v in old.items() if k_ not in doc})

    if args.default_path:
        this, parent = args.default_path[0::2], args.default_path[1::2]
        doc["default_path"] = dict(
            what="python bench.py --gpus 1 --steps 3 --warmup 1, this tree and the parent commit alternated in one session (this, parent, ...)",
            this_reads_per_s=[round(v) for v in this], parent_reads_per_s=[round(v) for v in parent], this_mean=round(sum(this) / 3),
            parent_mean=round(sum(parent) / 3), spread_this=round(max(this) - min(this)), spread_parent=round(max(parent) - min(parent)))
    # the host comparisons run on the cores the measurement allows: OMP_NUM_THREADS where it is set (scikit-learn reads it itself)
    host_threads = int(os.environ.get("OMP_NUM_THREADS") or min(16, len(os.sched_getaffinity(0))))

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")

    save()
    ctx = _lib.default_context()
    L = _lib.load()
    T, D, B = args.trees, args.depth, args.borders
    for name in args.shapes:
        n, F, k = SHAPES[name]
        Xtr, ytr, Xte, yte = make_rows(n, F, k, 7)
        acc = lambda pred: float((np.asarray(pred) == yte).mean())   # noqa: E731
        t0 = time.time()
        _boost_fit.borders(Xtr, B)
        t_borders = time.time() - t0
        t0 = time.time()
        first = device_fit(Xtr, ytr, min(T, 20), D, B)     # sizes the context's buffers, loads the kernels
        t_first = time.time() - t0
        _lib.check(L.wdx_kernel_timing(ctx.handle, 1))
        _lib.check(L.wdx_kernel_time_reset(ctx.handle))
        t0 = time.time()
        dev = device_fit(Xtr, ytr, T, D, B)
        t_dev = time.time() - t0
        ms, launches = C.c_double(0), C.c_int64(0)
        _lib.check(L.wdx_kernel_time(ctx.handle, _lib.K_BOOST_FIT, C.byref(ms), C.byref(launches)))
        _lib.check(L.wdx_kernel_timing(ctx.handle, 0))
        assert np.array_equal(first._leaf_values, dev._leaf_values[:first._leaf_values.size]), "two device fits of the same data differ"
        assert np.array_equal(dev.predict_raw(Xtr[:4096])[0], dev.train_scores[:4096]), "the tail does not return the trainer's scores"
        rec = dict(shape=name, rows=n, features=F, n_classes=k, trees=T, depth=D, border_count=B, learning_rate=LR, l2_leaf_reg=LAM,
                   host_cpus=len(os.sched_getaffinity(0)), host_threads=host_threads,
                   device=dict(borders_host_s=round(t_borders, 3), fit_call_s=round(t_dev, 3), first_call_20_trees_s=round(t_first, 3),
                               launches_ms=round(ms.value, 2), launches=int(launches.value), ms_per_tree=round(ms.value / T, 4),
                               held_out_accuracy=acc(dev.predict(Xte)[0])))
        if args.split_trees:
            rec["split"] = kernel_split(name, args.split_trees, D, B)
        if not args.no_host:
            HT = args.host_trees or T
            try:
                from sklearn.ensemble import HistGradientBoostingClassifier

                t0 = time.time()
                hgb = HistGradientBoostingClassifier(max_iter=HT, max_depth=D, max_bins=min(B, 255), learning_rate=LR, l2_regularization=LAM,
                                                     max_leaf_nodes=None, early_stopping=False).fit(Xtr, ytr)
                t_h = time.time() - t0
                rec["sklearn_hist_gradient_boosting"] = dict(
                    iterations=HT, trees_built=HT * (k if k > 2 else 1), fit_s=round(t_h, 3), ms_per_iteration=round(1e3 * t_h / HT, 3),
                    held_out_accuracy=acc(hgb.predict(Xte)), note="leaf-wise trees, one per class and iteration: a different algorithm")
                rec["sklearn_ms_per_iteration_over_device_ms_per_tree"] = round((1e3 * t_h / HT) / (ms.value / T), 2)
            except ImportError as e:
                rec["sklearn_hist_gradient_boosting"] = dict(error=repr(e))
            try:
                from catboost import CatBoostClassifier

                t0 = time.time()
                cb = CatBoostClassifier(iterations=HT, depth=D, learning_rate=LR, l2_leaf_reg=LAM, border_count=B, loss_function="MultiClass",
                                        thread_count=host_threads, verbose=False).fit(Xtr, ytr)
                t_c = time.time() - t0
                rec["catboost"] = dict(iterations=HT, fit_s=round(t_c, 3), ms_per_iteration=round(1e3 * t_c / HT, 3),
                                       held_out_accuracy=acc(np.asarray(cb.predict(Xte)).ravel()))
            except ImportError as e:
                rec["catboost"] = dict(error="not importable here: " + repr(e))
        print(json.dumps(rec), flush=True)
        doc["shapes"].append(rec)
        save()   # (after every shape: a run that is cut short keeps what it measured)


if __name__ == "__main__":
    main()
