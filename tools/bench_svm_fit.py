#!/usr/bin/env python3
"""What `DTW_SVM.fit` costs behind the self-distance matrix on one MI355X, with both solvers on the SAME distances:

  libsvm   scikit-learn's `SVC(kernel="precomputed", probability=True)` on one host core: the k (k - 1) / 2 one-vs-one problems and
           the five fold problems of each, one after the other (`fit(solver="libsvm")`: the code as it was before the device solver)
  device   `fit(solver="device")`: all of them in one launch of the SMO kernel (wdx_svm_fit.hip), K uploaded for the call,
           `sigmoid_train` and the assembly on the host

Workloads: 4 096 and 16 384 rows x 10 classes at L 25 and L 110, window 15, penalty 0.1, C = 1, class_weight = "balanced", tol 1e-3
(the recipe of the shipped models); noisy rows around ten centres, so that most rows are support vectors.  The distances are
computed once per workload (`parallel_distances.self_distance_matrix`) and handed to both fits.  Per workload: wall time of each
fit (the device fit twice: the first call sizes the context's buffers and loads the kernel), the solve launch alone (the
library's event pair, WDX_K_SVM_FIT), iterations per problem, the largest differences of the models' pairwise decision values on
held-out rows and of probA / probB (the folds differ: `_svm_fit`), the worst KKT residual of each model, and held-out accuracy.

    python tools/bench_svm_fit.py --out profiles/svm_fit.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WINDOW, PENALTY, N_CLASSES, N_TEST = 15, 0.1, 10, 2048
# -Rpass-analysis=kernel-resource-usage of wdx_svm_fit.hip (gfx950): VGPRs, scratch bytes / lane, dynamic LDS bytes / workgroup
KERNEL_RESOURCES = {
    "svm_fit_kernel<64, 4>": dict(vgprs=64, scratch=0, lds=3072),
    "svm_fit_kernel<256, 8>": dict(vgprs=70, scratch=0, lds=17408),
    "svm_fit_kernel<1024, 16>": dict(vgprs=124, scratch=0, lds=132096),
}


def make_rows(n, L, seed):
    rng = np.random.default_rng(seed)
    centres = np.cumsum(rng.normal(0, 0.3, (N_CLASSES, L)), axis=1)
    y = rng.integers(0, N_CLASSES, n + N_TEST)
    X = centres[y] + 0.5 * rng.normal(size=(n + N_TEST, L))
    return X[:n], y[:n], X[n:], y[n:]


def pair_decisions(model, Kq):
    """(n, pairs) one-vs-one decision values of kernel rows Kq (n, n_train), libsvm's layout"""
    start = np.r_[0, np.cumsum(model._n_support)]
    Ks = Kq[:, model._support]
    out, p, k = [], 0, len(model._n_support)
    for i in range(k):
        for j in range(i + 1, k):
            si, sj = slice(start[i], start[i + 1]), slice(start[j], start[j + 1])
            out.append(Ks[:, si] @ model._dual_coef[j - 1, si] + Ks[:, sj] @ model._dual_coef[i, sj] - model._rho[p])
            p += 1
    return np.stack(out, axis=1)


def kkt_of(model, D, w):
    from helpers import kkt

    sup = model._support
    return kkt.worst(kkt.kkt_residuals(D[np.ix_(sup, sup)], model._n_support, model._dual_coef, -model._rho, w))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 16384])
    ap.add_argument("--lengths", type=int, nargs="*", default=[25, 110])
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from warpdemux_amd import _lib
    from warpdemux_amd import parallel_distances as pdist
    from warpdemux_amd.models import DTW_SVM

    ctx, lib = _lib.default_context(), _lib.load()
    results = []
    for L in args.lengths:
        for n in args.sizes:
            Xtr, y, Xte, yte = make_rows(n, L, 100 * L + n % 997)
            t0 = time.time()
            D = pdist.self_distance_matrix(Xtr, WINDOW, PENALTY)
            t_dist = time.time() - t0
            kw = dict(distances=D, class_weight="balanced", C=1.0, tol=1e-3)
            t0 = time.time()
            first = DTW_SVM.fit(Xtr, y, WINDOW, PENALTY, solver="device", **kw)
            t_first = time.time() - t0
            _lib.check(lib.wdx_kernel_timing(ctx.handle, 1))
            _lib.check(lib.wdx_kernel_time_reset(ctx.handle))
            t0 = time.time()
            dev = DTW_SVM.fit(Xtr, y, WINDOW, PENALTY, solver="device", **kw)
            t_dev = time.time() - t0
            ms, launches = C.c_double(0), C.c_int64(0)
            _lib.check(lib.wdx_kernel_time(ctx.handle, _lib.K_SVM_FIT, C.byref(ms), C.byref(launches)))
            _lib.check(lib.wdx_kernel_timing(ctx.handle, 0))
            assert np.array_equal(first._dual_coef, dev._dual_coef), "two device fits of the same data differ"
            t0 = time.time()
            ref = DTW_SVM.fit(Xtr, y, WINDOW, PENALTY, solver="libsvm", **kw)
            t_ref = time.time() - t0
            info = dev.fit_info_
            w = n / (N_CLASSES * np.bincount(y, minlength=N_CLASSES).astype(np.float64))
            Kq = np.exp(-pdist.distance_matrix_to(Xte, Xtr, window=WINDOW, penalty=PENALTY, n_jobs=1)).astype(np.float64)
            d_dev, d_ref = pair_decisions(dev, Kq), pair_decisions(ref, Kq)
            acc = lambda m: float((np.asarray(m.predict(Xte, nproc=1)[0]) == yte).mean())   # noqa: E731
            full = info["fold"] == -1
            rec = dict(L=L, n=n, n_classes=N_CLASSES, window=WINDOW, penalty=PENALTY, problems=int(len(info["state"])),
                       rows_per_problem=dict(min=int(info["rows"].min()), max=int(info["rows"].max())),
                       self_distance_matrix_s=round(t_dist, 3), fit_libsvm_s=round(t_ref, 3), fit_device_s=round(t_dev, 3),
                       fit_device_first_call_s=round(t_first, 3), solve_launch_ms=round(ms.value, 3), solve_launches=int(launches.value),
                       libsvm_over_device=round(t_ref / t_dev, 2), states=sorted(set(int(s) for s in info["state"])),
                       iterations=dict(full_min=int(info["n_iter"][full].min()), full_max=int(info["n_iter"][full].max()),
                                       fold_min=int(info["n_iter"][~full].min()), fold_max=int(info["n_iter"][~full].max()),
                                       per_row_mean=round(float((info["n_iter"] / info["rows"]).mean()), 3), total=int(info["n_iter"].sum())),
                       us_per_iteration_of_the_longest_problem=round(1e3 * ms.value / max(1, int(info["n_iter"].max())), 3),
                       support_rows=dict(device=int(len(dev._support)), libsvm=int(len(ref._support))),
                       max_abs_decision_difference=float(np.abs(d_dev - d_ref).max()),
                       max_abs_probA_difference=float(np.abs(dev._probA - ref._probA).max()),
                       max_abs_probB_difference=float(np.abs(dev._probB - ref._probB).max()),
                       kkt_worst=dict(device=kkt_of(dev, D, w), libsvm=kkt_of(ref, D, w)),
                       held_out_accuracy=dict(device=acc(dev), libsvm=acc(ref)))
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del D, Kq
            if args.out:   # (after every workload: a run that is cut short keeps what it measured)
                doc = dict(tool="tools/bench_svm_fit.py", device=torch.cuda.get_device_name(0), kernel_resources=KERNEL_RESOURCES, shapes=results)
                with open(args.out, "w") as f:
                    json.dump(doc, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
