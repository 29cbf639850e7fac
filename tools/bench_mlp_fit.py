#!/usr/bin/env python3
"""What `DTW_MLP.fit` costs behind the distance matrix on one MI355X, with both solvers on the SAME float32 distances, the same seed
and the same number of epochs:

  sklearn  `fit(solver="sklearn")`: the StandardScaler + MLPClassifier(solver="adam") pipeline on the host cores the process may use
  device   `fit(solver="device")`: the engine's trainer (wdx_mlp_fit.hip), the matrix uploaded for the call, 2 n_layers launches per
           minibatch, one synchronisation per epoch

Shapes, both with ten classes and hidden (100,), batch 200 (scikit-learn's "auto"):
  consensus  40 references x 110 points, 30 000 rows
  wdx10      2 601 references x 25 points, 16 384 rows
Rows are noisy copies of ten templates; the references are noisy copies too (what matters here is the matrix's shape).  Per shape:
wall time per epoch of each fit (the device fit twice: the first call sizes the context's buffers and loads the kernels), the
trainer's launches alone (the library's event pairs, WDX_K_MLP_FIT), launches per step, the largest difference of the two models'
parameters, and held-out accuracy of both.  `--accuracy` also writes the figures of every accuracy case of
tests/test_gpu_mlp_fit.py (device error / E_ref).

    python tools/bench_mlp_fit.py --out profiles/mlp_fit.json --accuracy profiles/mlp_fit_accuracy.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WINDOW, PENALTY, N_CLASSES, N_TEST, HIDDEN = 15, 0.1, 10, 2048, (100,)
SHAPES = {"consensus": (40, 110, 30000), "wdx10": (2601, 25, 16384)}


def make_rows(n_refs, L, n, seed):
    rng = np.random.default_rng(seed)
    templates = np.cumsum(rng.normal(0, 0.3, (N_CLASSES, L)), axis=1)
    y = rng.integers(0, N_CLASSES, n + N_TEST)
    X = templates[y] + 0.5 * rng.normal(size=(n + N_TEST, L))
    refs = templates[np.arange(n_refs) % N_CLASSES] + 0.3 * rng.normal(size=(n_refs, L))
    return X[:n], y[:n], X[n:], y[n:], refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--accuracy", default="")
    args = ap.parse_args()

    import torch

    from warpdemux_amd import _lib
    from warpdemux_amd import parallel_distances as pdist
    from warpdemux_amd.engine import DemuxEngine
    from warpdemux_amd.models import DTW_MLP

    if args.accuracy:
        import test_gpu_mlp_fit as t

        t._imports()
        eng = DemuxEngine(np.zeros((1, 25)), WINDOW, PENALTY)
        cases = [t.measure(eng, name) for name in t.CASES]
        eng.close()
        with open(args.accuracy, "w") as f:
            json.dump(dict(tool="tools/bench_mlp_fit.py --accuracy", device=torch.cuda.get_device_name(0),
                           contract="T = 4 max(E_ref, 2^-24 max|theta|); E_ref = max |scikit-learn float32 - scikit-learn float64|; "
                                    "ratio_to_e_ref = max |device - scikit-learn float64| / E_ref (the contract allows 4 where E_ref is the "
                                    "larger term), ratio_to_T the same error / T (the contract allows 1); ratio_loss and ratio_loss_to_T: "
                                    "the loss curve's; hyper: the case's hyper-parameters beyond scikit-learn's defaults",
                           cases=cases), f, indent=1)
            f.write("\n")

    ctx = _lib.default_context()
    results = []
    for name in args.shapes:
        n_refs, L, n = SHAPES[name]
        Xtr, y, Xte, yte, refs = make_rows(n_refs, L, n, 7 + n_refs)
        t0 = time.time()
        D = pdist.distance_matrix_to(Xtr, refs, window=WINDOW, penalty=PENALTY, n_jobs=1)
        t_dist = time.time() - t0
        E = args.epochs
        kw = dict(refs=refs, hidden_layer_sizes=HIDDEN, max_iter=E, tol=1e-12, n_iter_no_change=E + 1, random_state=1, distances=D)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            t0 = time.time()
            first = DTW_MLP.fit(Xtr, y, WINDOW, PENALTY, solver="device", **kw)
            t_first = time.time() - t0
            _lib.check(_lib.load().wdx_kernel_timing(ctx.handle, 1))
            _lib.check(_lib.load().wdx_kernel_time_reset(ctx.handle))
            t0 = time.time()
            dev = DTW_MLP.fit(Xtr, y, WINDOW, PENALTY, solver="device", **kw)
            t_dev = time.time() - t0
            ms, launches = C.c_double(0), C.c_int64(0)
            _lib.check(_lib.load().wdx_kernel_time(ctx.handle, _lib.K_MLP_FIT, C.byref(ms), C.byref(launches)))
            _lib.check(_lib.load().wdx_kernel_timing(ctx.handle, 0))
            t0 = time.time()
            ref = DTW_MLP.fit(Xtr, y, WINDOW, PENALTY, solver="sklearn", **kw)
            t_ref = time.time() - t0
        assert all(np.array_equal(a, b) for a, b in zip(first._coefs, dev._coefs)), "two device fits of the same data differ"
        assert dev.n_iter_ == ref.n_iter_ == E
        steps = -(-n // min(200, n))
        acc = lambda m: float((np.asarray(m.predict(Xte, nproc=1)[0]) == yte).mean())   # noqa: E731
        rec = dict(shape=name, n_refs=n_refs, L=L, rows=n, n_classes=N_CLASSES, hidden=list(HIDDEN), batch=200, epochs=E,
                   host_cpus=len(os.sched_getaffinity(0)), omp_num_threads=os.environ.get("OMP_NUM_THREADS"),
                   distance_matrix_s=round(t_dist, 3), fit_sklearn_s=round(t_ref, 3), fit_device_s=round(t_dev, 3),
                   fit_device_first_call_s=round(t_first, 3), sklearn_ms_per_epoch=round(1e3 * t_ref / E, 2),
                   device_ms_per_epoch=round(1e3 * t_dev / E, 2), device_launches_ms_per_epoch=round(ms.value / E, 3),
                   launches=int(launches.value), steps_per_epoch=steps, launches_per_step=int(launches.value) // (E * steps),
                   sklearn_over_device=round(t_ref / t_dev, 2),
                   max_abs_parameter_difference=float(max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(dev._coefs + dev._intercepts,
                                                                                                                   ref._coefs + ref._intercepts))),
                   final_loss=dict(device=float(dev.loss_curve_[-1]), sklearn=float(ref.loss_curve_[-1])),
                   held_out_accuracy=dict(device=acc(dev), sklearn=acc(ref)))
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del D
        if args.out:   # (after every shape: a run that is cut short keeps what it measured)
            with open(args.out, "w") as f:
                json.dump(dict(tool="tools/bench_mlp_fit.py", device=torch.cuda.get_device_name(0), shapes=results), f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
