#!/usr/bin/env python3
"""Host time of the three model setters (wdx_svm_set_model, wdx_mlp_set_model, wdx_boost_set_model) on an idle context, this
tree's library against another build of it (a parent checkout's libwdx_hip.so), on one MI355X.

Models of shipped size: the WDX4 SVM of tests/golden/g6_dtw_svm_wdx4.npz (851 support vectors, 5 classes) and the WDX10 SVM of
tests/golden/g9_kkt_models.npz (2 601 support vectors, 11 classes; the file holds no Platt parameters or support indices:
drawn / the identity -- the setter's time does not depend on their values); no MLP or boost model ships as a fixture, so an
MLP over the WDX10 distances (2 601 inputs, 100 hidden units, 11 classes, float32: 1.05 MB) and CatBoost's default forest
(1 000 trees of depth 6, 4 classes, 25 features: 2.1 MB) are built at those sizes.

A run is one fresh process with one library: a context, every model set once (warm), then `--calls` timed calls of each
setter, nothing in flight; the run's figure is the median per setter.  `--runs` runs a side, the two libraries alternating.
Per setter and side: the median of the runs' figures and their range.

    python tools/bench_model_install.py --parent-lib <parent checkout>/warpdemux_amd/csrc/libwdx_hip.so --out profiles/model_install.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SETTERS = {"svm_wdx4": "wdx_svm_set_model", "svm_wdx10": "wdx_svm_set_model", "mlp_wdx10": "wdx_mlp_set_model",
           "boost_1000x6x4": "wdx_boost_set_model"}


def build_models():
    from warpdemux_amd import models

    rng = np.random.default_rng(7)
    g6 = np.load(os.path.join(GOLDEN, "g6_dtw_svm_wdx4.npz"))
    wdx4 = models.DTW_SVM(g6["X_train"], g6["n_support"], g6["support"], g6["dual_coef"], -g6["intercept"], g6["probA"], g6["probB"],
                          {int(k): int(v) for k, v in zip(g6["label_keys"], g6["label_vals"])}, g6["thresholds"],
                          window=int(g6["window"]), penalty=float(g6["penalty"]), gamma=float(g6["gamma"]), pwr_dist=int(g6["pwr_dist"]))
    g9 = np.load(os.path.join(GOLDEN, "g9_kkt_models.npz"))
    X, ns, k = g9["WDX10__X"], g9["WDX10__n_support"], len(g9["WDX10__n_support"])
    npairs = k * (k - 1) // 2
    wdx10 = models.DTW_SVM(X, ns, np.arange(len(X), dtype=np.int32), g9["WDX10__dual_coef"], -g9["WDX10__intercept"],
                           -rng.uniform(0.3, 4.0, npairs), rng.normal(0, 0.5, npairs), {i: i for i in range(k)}, None,
                           window=int(g9["WDX10__window"]), penalty=float(g9["WDX10__penalty"]), gamma=float(g9["WDX10__gamma"]),
                           pwr_dist=int(g9["WDX10__pwr_dist"]))
    sizes = (len(X), 100, k)
    mlp = models.DTW_MLP(X, [rng.normal(0, 0.1, (a, b)).astype(np.float32) for a, b in zip(sizes[:-1], sizes[1:])],
                         [rng.normal(0, 0.1, b).astype(np.float32) for b in sizes[1:]], "relu", {i: i for i in range(k)}, None,
                         window=15, penalty=0.1)
    trees = [(rng.integers(0, 25, 6), rng.uniform(-1.5, 1.5, 6).astype(np.float32), [False] * 6, rng.normal(0, 0.1, (64, 4)))
             for _ in range(1000)]
    boost = models.Fpt_Boost(trees, 25, 1.0, np.zeros(4), {i: i for i in range(4)}, None)
    return {"svm_wdx4": wdx4, "svm_wdx10": wdx10, "mlp_wdx10": mlp, "boost_1000x6x4": boost}


def one_run(calls):
    """in a child: JSON {name: median seconds of one call} on stdout"""
    from warpdemux_amd import _lib

    L = _lib.load()
    ctx = _lib.Context(0)
    out = {}
    try:
        for name, model in build_models().items():
            m = model.to_c()
            setter = getattr(L, SETTERS[name])
            _lib.check(setter(ctx.handle, C.byref(m)))
            t = []
            for _ in range(calls):
                t0 = time.perf_counter()
                rc = setter(ctx.handle, C.byref(m))
                t.append(time.perf_counter() - t0)
                _lib.check(rc)
            out[name] = statistics.median(t)
    finally:
        ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libwdx_hip.so built from the parent commit")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--calls", type=int, default=21)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return one_run(a.calls)
    libs = {"this_tree": os.path.join(ROOT, "warpdemux_amd", "csrc", "libwdx_hip.so")}
    if a.parent_lib:
        libs = {"parent": os.path.abspath(a.parent_lib), **libs}
    runs = {side: [] for side in libs}
    for _ in range(a.runs):
        for side, lib in libs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls)],
                               env={**os.environ, "WDX_LIB_PATH": lib}, capture_output=True, text=True, timeout=120)
            if r.returncode != 0:      # nothing more is started on the device after a failed run
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                return r.returncode
            runs[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = {"what": "host time of one setter call on an idle context, microseconds; per run the median of `calls` calls, per side "
                   "the median and range of the runs' figures; the two libraries alternate run by run, a fresh process each",
           "runs_per_side": a.runs, "calls_per_run": a.calls, "sides": {}}
    for side, rr in runs.items():
        res["sides"][side] = {}
        for name in SETTERS:
            us = [1e6 * r[name] for r in rr]
            res["sides"][side][name] = {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2),
                                        "max_us": round(max(us), 2), "runs_us": [round(u, 2) for u in us]}
    if a.parent_lib:
        res["ratio_of_medians_this_tree_over_parent"] = {
            name: round(res["sides"]["this_tree"][name]["median_us"] / res["sides"]["parent"][name]["median_us"], 3) for name in SETTERS}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
