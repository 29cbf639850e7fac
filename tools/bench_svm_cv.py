#!/usr/bin/env python3
"""Measures the cross-validated probabilities and the accuracy thresholds -> profiles/svm_cv.json.

  cv          ten classes, L = 110, window 15: `DTW_SVM.cross_val_predict` (cv = 5: D, K and ONE solve on the device) against the
              same result assembled from what the engine had before it: one host self-distance matrix, five
              `DTW_SVM.fit(solver="device", distances=D[T][:, T])` and five `predict(X[H])`.  The two alternate (A B A B ..),
              each timed by the wall clock around a synchronised call; the median and the range of the rounds are reported,
              with the share of rows on which the two agree in the predicted class.
  kernels     on the resident matrix of that shape: the one solve's launch (WDX_K_SVM_FIT), the kernel matrix
              (WDX_K_SVM_KERNEL, with its share of the stated HBM bandwidth: 8 bytes per entry), the coupling
              (WDX_K_SVM_CV_COUPLE) and the thresholds (WDX_K_THRESHOLDS), by the library's own events
  thresholds  `DemuxEngine.accuracy_thresholds` on an (n, 10) float64 probability tensor that is already on the device, beside
              the time to copy that tensor to pageable host memory -- the alternative it replaces
  exp_rule    how far K from exp_rule lies from NumPy's float32 exp on the same distances (float32 ulps), and how far the
              decision values of the two fits on those two matrices lie apart

    python tools/bench_svm_cv.py [--rows 4096,16384] [--rounds 3] [--thr-rows 10000000] [--out profiles/svm_cv.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12   # MI355X: 8 TB/s peak
L, WINDOW, PENALTY, K_CLASSES, CV = 110, 15, 0.1, 10, 5


def fingerprints(m, seed=0):
    rng = np.random.default_rng(seed)
    proto = rng.normal(size=(K_CLASSES, L))
    y = rng.permutation(np.arange(m) % K_CLASSES)
    return np.ascontiguousarray(proto[y] + 1.0 * rng.normal(size=(m, L))), 3 + 2 * y


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(np.min(ts)), "max_s": float(np.max(ts)), "rounds": len(ts)}


def parent_route(models, pdist, _svm_cv, X, labels, gamma, args):
    """out-of-fold probabilities from fit + predict per fold (the folds are taken from `_svm_cv` so that both routes hold out the
    same rows)"""
    classes = np.unique(labels)
    y_idx = np.searchsorted(classes, labels)
    D = pdist.self_distance_matrix(X, window=WINDOW, penalty=PENALTY)
    _, train, held = _svm_cv.outer_folds(y_idx, len(classes), CV, args["random_state"])
    prob = np.empty((len(X), len(classes)))
    for T, H in zip(train, held):
        model = models.DTW_SVM.fit(X[T], labels[T], WINDOW, PENALTY, gamma=gamma, solver="device", distances=np.ascontiguousarray(D[T][:, T]), **args)
        prob[H] = model.predict(X[H], nproc=1)[1]
    return prob


def bench_cv(m, rounds, out):
    import torch

    from warpdemux_amd import _lib, _svm_cv, _svm_fit, models
    from warpdemux_amd import parallel_distances as pdist
    from warpdemux_amd.engine import DemuxEngine

    X, labels = fingerprints(m)
    args = dict(C=1.0, class_weight="balanced", tol=1e-3, random_state=0)
    D0 = pdist.self_distance_matrix(X[:512], window=WINDOW, penalty=PENALTY)
    gamma = float(np.float32(1.5 / np.median(D0[D0 > 0])))
    change = lambda: models.DTW_SVM.cross_val_predict(X, labels, WINDOW, PENALTY, gamma=gamma, cv=CV, **args)   # noqa: E731
    parent = lambda: parent_route(models, pdist, _svm_cv, X, labels, gamma, args)                                # noqa: E731
    change(), parent()   # warm: kernels loaded, workspaces sized
    t_change, t_parent = [], []
    for _ in range(rounds):
        for fn, ts in ((parent, t_parent), (change, t_change)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            if fn is parent:
                p_parent = res
            else:
                p_change = res[0]
    agree = float((np.argmax(p_parent, axis=1) == np.argmax(p_change, axis=1)).mean())
    row = {"rows": m, "classes": K_CLASSES, "L": L, "window": WINDOW, "cv": CV, "gamma": gamma, "cross_val_predict": stats(t_change),
           "parent_fit_predict_per_fold": stats(t_parent), "same_predicted_class": agree,
           "max_abs_probability_difference": float(np.nanmax(np.abs(p_parent - p_change)))}

    # the kernels alone, by the library's events, on the resident matrix
    eng = DemuxEngine(np.zeros((1, L)), 15, 0.1)
    try:
        classes = np.unique(labels)
        y_idx = np.searchsorted(classes, labels)
        Xd = torch.tensor(X, device="cuda")
        D = eng.self_distances(Xd, WINDOW, PENALTY)
        Dh = D.cpu().numpy()
        K = eng.svm_kernel(D, gamma)
        eng.svm_cross_val(K, y_idx, K_CLASSES, cv=CV, **args)
        eng.kernel_timing(True)
        eng.kernel_time_reset()
        reps = 5
        for _ in range(reps):
            eng.svm_kernel(D, gamma, out=K)
        res = eng.svm_cross_val(K, y_idx, K_CLASSES, cv=CV, **args)
        yd = torch.tensor(y_idx.astype(np.int32), device="cuda")
        for _ in range(reps):
            eng.accuracy_thresholds(res.prob, yd, (0.95, 0.99, 0.999))
        torch.cuda.synchronize()
        ms_kernel = eng.kernel_time(_lib.K_SVM_KERNEL)[0] / reps
        row["kernels_ms"] = {"svm_fit_launch": eng.kernel_time(_lib.K_SVM_FIT)[0], "svm_kernel": ms_kernel,
                             "svm_cv_couple": eng.kernel_time(_lib.K_SVM_CV_COUPLE)[0], "thresholds": eng.kernel_time(_lib.K_THRESHOLDS)[0] / reps,
                             "problems_in_the_launch": int(len(res.plan.batch.problems))}
        row["svm_kernel_hbm_share"] = 8.0 * m * m / (ms_kernel * 1e-3) / HBM_BYTES_PER_S
        eng.kernel_timing(False)
        # exp_rule against numpy.exp on the same float32 distances
        Kh = K.cpu().numpy()
        Kn = np.exp(-np.float32(gamma) * Dh)
        a, b = Kh.view(np.int32).astype(np.int64), Kn.view(np.int32).astype(np.int64)
        row["exp_rule_vs_numpy_exp"] = {"max_ulp_float32": int(np.abs(a - b).max()), "entries_that_differ": int((a != b).sum()), "entries": int(m * m)}
        w = _svm_fit.class_weights("balanced", classes, y_idx)
        batch = _svm_fit.build_batch(y_idx, K_CLASSES, 1.0 * w, 0, folds=False)
        ev = np.arange(0, m, max(1, m // 512), dtype=np.int32)   # decision values of every pair on a sample of rows
        tab = batch.problems.copy()
        tab["eval0"] = np.arange(len(tab)) * len(ev)
        tab["n_eval"] = len(ev)
        evs = np.tile(ev, len(tab))
        d1 = eng.svm_solve(K, tab, batch.rows, evs, eps=1e-3).dec.cpu().numpy()
        d2 = eng.svm_solve(torch.tensor(Kn, device="cuda"), tab, batch.rows, evs, eps=1e-3).dec.cpu().numpy()
        row["exp_rule_vs_numpy_exp"]["max_abs_decision_value_difference"] = float(np.abs(d1 - d2).max())
        row["exp_rule_vs_numpy_exp"]["decision_values_compared"] = int(d1.size)
    finally:
        eng.close()
    out["cv"].append(row)
    print(json.dumps(row))


def bench_thresholds(n, out):
    import torch

    from warpdemux_amd.engine import DemuxEngine

    eng = DemuxEngine(np.zeros((1, 25)), 15, 0.1)
    try:
        g = torch.Generator(device="cuda").manual_seed(1)
        prob = torch.softmax(3.0 * torch.randn((n, K_CLASSES), dtype=torch.float64, device="cuda", generator=g), dim=1)
        y = torch.randint(0, K_CLASSES, (n,), dtype=torch.int32, device="cuda", generator=g)
        eng.accuracy_thresholds(prob, y, (0.95, 0.99, 0.999))
        torch.cuda.synchronize()
        t_dev, t_copy = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            eng.accuracy_thresholds(prob, y, (0.95, 0.99, 0.999))
            torch.cuda.synchronize()
            t_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            prob.cpu()
            t_copy.append(time.perf_counter() - t0)
        row = {"rows": n, "classes": K_CLASSES, "resolution": 100, "targets": 3, "accuracy_thresholds": stats(t_dev),
               "copy_probabilities_to_host": stats(t_copy), "bytes": int(prob.numel() * 8),
               "hbm_share": prob.numel() * 8 / float(np.median(t_dev)) / HBM_BYTES_PER_S}
    finally:
        eng.close()
    out["thresholds"] = row
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,16384")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--thr-rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svm_cv.json"))
    a = ap.parse_args()
    out = {"tool": "tools/bench_svm_cv.py", "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "cv": []}
    bench_thresholds(a.thr_rows, out)
    for m in [int(v) for v in a.rows.split(",") if v]:
        bench_cv(m, a.rounds, out)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
