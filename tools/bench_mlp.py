"""DTW_MLP tail: the parent commit's way of running a DTW_MLP against the device tail.

    python tools/bench_mlp.py [--out profiles/NAME.json] [--parent-tree DIR] [--reads-wdx10 N] [--reads-consensus N]

Two shapes, each with a float32 MLPClassifier (hidden (100,), k 11) fitted for one iteration on float32 distances and given
random weights (the timing does not depend on their values):
  - WDX10-size: 2 601 references x 25 points, window 15;
  - consensus:  40 references x 110 points, window 15.
Legs, timed in the same process session on the same reads:
  (a) the parent commit's path: our distance_matrix_to to the host, then scikit-learn predict_proba + process_probs on the
      host CPUs.  Run in a child process against --parent-tree (a checkout of the parent commit with its library built), so
      that it uses only what existed there;
  (b) warpdemux_amd.models.DTW_MLP.predict on the same host fingerprints;
  (c) DemuxEngine.demux_mlp device-resident on synthetic reads (fingerprint -> DTW row blocks -> MLP tail).
Also reported: the MLP kernel's share of the DTW kernel time (WDX_K_MLP / WDX_K_DTW in leg b) and its rate against the
f32 matrix peak and HBM (the benchmarked models are float32).  One JSON document on stdout (and in --out).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"wdx10": dict(nY=2601, L=25, window=15), "consensus": dict(nY=40, L=110, window=15)}
HIDDEN, K, PENALTY = (100,), 11, 0.1
PEAK_F32_MATRIX, PEAK_HBM = 157.3e12, 8.0e12   # MI355X spec sheet


def _model(nY, dtype, seed=0):
    import warnings

    from sklearn.neural_network import MLPClassifier

    rng = np.random.default_rng(seed)
    m = MLPClassifier(hidden_layer_sizes=HIDDEN, max_iter=1, random_state=seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(rng.uniform(2, 8, size=(2 * K, nY)).astype(dtype), np.arange(2 * K) % K)
    m.coefs_ = [rng.normal(0, np.sqrt(2 / sum(W.shape)), W.shape).astype(dtype) for W in m.coefs_]
    m.intercepts_ = [rng.normal(0, np.sqrt(0.1), b.shape).astype(dtype) for b in m.intercepts_]
    return m


def _data(shape, n, seed=1):
    s = SHAPES[shape]
    rng = np.random.default_rng(seed)
    refs = rng.normal(size=(s["nY"], s["L"]))
    X = refs[rng.integers(0, s["nY"], n)] + rng.normal(0, 0.7, size=(n, s["L"]))
    return refs, X


def _process_probs(y_prob, label_mapper, thresholds=None):
    """models/utils.py:45-61"""
    pred_idx = np.argmax(y_prob, axis=1)
    pred = np.array([label_mapper[i] for i in pred_idx])
    srt = np.sort(y_prob, axis=1)[:, ::-1]
    conf = srt[:, 0] - srt[:, 1]
    if thresholds is not None:
        pred[conf < thresholds[pred_idx]] = -1
    return pred, conf


def leg_a(shape, n, reps):
    """the parent's path (imports whatever warpdemux_amd is first on sys.path: the parent tree in the child process)"""
    from warpdemux_amd.parallel_distances import distance_matrix_to

    refs, X = _data(shape, n)
    m = _model(refs.shape[0], np.float32)
    lm = {i: i for i in range(K)}
    w = SHAPES[shape]["window"]
    D = distance_matrix_to(X, refs, window=w, penalty=PENALTY, n_jobs=1)   # warm-up
    m.predict_proba(D)
    t0 = time.perf_counter()
    for _ in range(reps):
        D = distance_matrix_to(X, refs, window=w, penalty=PENALTY, n_jobs=1)
        t1 = time.perf_counter()
        pred, _ = _process_probs(m.predict_proba(D), lm)
    dt = (time.perf_counter() - t0) / reps
    return dict(seconds=dt, reads_per_s=n / dt, distance_seconds=t1 - t0 - (reps - 1) * dt, pred_head=pred[:8].tolist())


def leg_bc(shape, n, reps, n_demux):
    import ctypes as C

    import torch

    from warpdemux_amd import _lib, models, sig_proc, synth
    from warpdemux_amd.engine import DemuxEngine

    refs, X = _data(shape, n)
    nY, L, w = refs.shape[0], refs.shape[1], SHAPES[shape]["window"]
    m = _model(nY, np.float32)

    class DTW_MLP:   # the upstream attributes (models/dtw_base.py:14-25)
        pass

    r = DTW_MLP()
    r.model, r._X, r.label_mapper, r.thresholds = m, refs, {i: i for i in range(K)}, None
    r.window, r.penalty, r.block_size, r.n_classes, r.noise_class = w, PENALTY, 1000, None, False
    dm = models.from_reference(r)
    dm.predict(X)   # warm-up + upload
    ctx = _lib.default_context()
    L_ = _lib.load()
    _lib.check(L_.wdx_kernel_timing(ctx.handle, 1))
    _lib.check(L_.wdx_kernel_time_reset(ctx.handle))
    t0 = time.perf_counter()
    for _ in range(reps):
        pred, _ = dm.predict(X)
    dt_b = (time.perf_counter() - t0) / reps

    def ktime(kid):
        ms, nl = C.c_double(0), C.c_int64(0)
        _lib.check(L_.wdx_kernel_time(ctx.handle, kid, C.byref(ms), C.byref(nl)))
        return ms.value / reps, nl.value

    mlp_ms, mlp_launches = ktime(_lib.K_MLP)
    dtw_ms, _ = ktime(_lib.K_DTW)
    _lib.check(L_.wdx_kernel_timing(ctx.handle, 0))
    flops = 2.0 * n * (nY * HIDDEN[0] + HIDDEN[0] * K)
    b = dict(seconds=dt_b, reads_per_s=n / dt_b, pred_head=pred[:8].tolist(), mlp_kernel_ms=mlp_ms,
             mlp_launches_per_call=mlp_launches / reps, dtw_kernel_ms=dtw_ms, mlp_share_of_dtw=mlp_ms / dtw_ms if dtw_ms else None,
             mlp_tflops=flops / (mlp_ms * 1e-3) / 1e12 if mlp_ms else None,
             mlp_frac_f32_matrix_peak=flops / (mlp_ms * 1e-3) / PEAK_F32_MATRIX if mlp_ms else None,
             mlp_hbm_frac=(4.0 * n * nY) / (mlp_ms * 1e-3) / PEAK_HBM if mlp_ms else None)

    # (c) device-resident on synthetic reads; the model's references are the engine's
    spec = synth.SynthSpec(n_barcodes=8)
    eng = DemuxEngine(refs, w, PENALTY, sig_proc.SegParams(barcode_num_events=L))
    eng.set_mlp(dm)
    sig, off, a_s, a_e, _, max_len = eng.synth_packed(spec, 0, n_demux)
    out = eng.demux_mlp(sig, a_s, a_e, offsets=off, max_len=max_len)
    torch.cuda.synchronize()
    eng.kernel_timing(True)
    eng.kernel_time_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = eng.demux_mlp(sig, a_s, a_e, offsets=off, max_len=max_len, out=out)
    torch.cuda.synchronize()
    dt_c = (time.perf_counter() - t0) / reps
    c = dict(seconds=dt_c, reads_per_s=n_demux / dt_c, n_reads=n_demux,
             fingerprint_ms=eng.kernel_time(_lib.K_FINGERPRINT)[0] / reps, dtw_ms=eng.kernel_time(_lib.K_DTW)[0] / reps,
             mlp_ms=eng.kernel_time(_lib.K_MLP)[0] / reps, ok_reads=int((out[3] == 0).sum().item()))
    eng.close()
    return b, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parent-tree", help="checkout of the parent commit with its library built (leg a)")
    ap.add_argument("--reads-wdx10", type=int, default=20000)
    ap.add_argument("--reads-consensus", type=int, default=200000)
    ap.add_argument("--demux-reads", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg-a", help=argparse.SUPPRESS)   # child mode: SHAPE,N,REPS
    args = ap.parse_args()
    if args.leg_a:
        shape, n, reps = args.leg_a.split(",")
        print(json.dumps(leg_a(shape, int(n), int(reps))))
        return
    sys.path.insert(0, ROOT)
    res = dict(tool="tools/bench_mlp.py", hidden=list(HIDDEN), k=K, dtype="float32", shapes={})
    for shape, n in (("wdx10", args.reads_wdx10), ("consensus", args.reads_consensus)):
        row = dict(SHAPES[shape], n_reads=n)
        if args.parent_tree:
            env = dict(os.environ, PYTHONPATH=os.path.abspath(args.parent_tree))
            env.pop("WDX_LIB_PATH", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg-a", f"{shape},{n},{args.reps}"],
                               cwd=os.path.abspath(args.parent_tree), env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"leg (a) failed:\n{p.stderr[-3000:]}")
            row["a_parent_host_sklearn"] = json.loads(p.stdout.strip().splitlines()[-1])
        row["b_DTW_MLP_predict"], row["c_demux_mlp"] = leg_bc(shape, n, args.reps, args.demux_reads)
        if "a_parent_host_sklearn" in row:
            a = row["a_parent_host_sklearn"]["reads_per_s"]
            row["speedup_b_over_a"] = row["b_DTW_MLP_predict"]["reads_per_s"] / a
            row["speedup_c_over_a"] = row["c_demux_mlp"]["reads_per_s"] / a
            row["same_preds_a_b"] = row["a_parent_host_sklearn"]["pred_head"] == row["b_DTW_MLP_predict"]["pred_head"]
        res["shapes"][shape] = row
        print(json.dumps({shape: row}), file=sys.stderr)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
