#!/usr/bin/env python3
"""Rate of the boundary detection (DemuxEngine.detect: wdx_detect_rows / wdx_detect_rows_adc) on one MI355X.

Resident reads of `--trace` samples each (default 1 M reads of 10 000 samples), generated on the device in the shape of the
synthetic traces of tests/helpers/detect_rule.py (open pore | adapter events | polyA | body; event boundaries on a grid of 40
samples), as float32 rows and as the int16 shard whose calibration gives exactly those rows.  Both forms are compared once
(every output, bit for bit), then timed in alternation with device events: two warm-up rounds, `--reps` timed ones.  Recorded:
median / min / max ms and reads/s of each, the kernel's own time from the library's event brackets (a run of its own), the
HBM floor (input bytes / 8 TB/s, MI355X peak) and the share of it reached, the codes the rule returned, and -- beside them --
the rate of the NumPy restatement on this host's granted cores (16 worker processes).

The timed window is one `DemuxEngine.detect` call -- its six output allocations and the launch -- so `method_reads_per_s` is the
method's rate; `kernel_reads_per_s` and the share of the HBM floor come from `kernel_ms`, the kernel alone.  The restatement is
the tests' own (`tests/helpers/detect_rule.py`, imported from the test tree: the tool needs a source checkout).

    python tools/bench_detect.py --out profiles/detect.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_BYTES_PER_S = 8.0e12


def generate(torch, n, trace, dev, chunk=20_000, seed=3):
    """(sig float32 (n, trace), adc int16 (n, trace), offset, scale): sig IS the calibration of adc, float32 add then multiply"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    sig = torch.empty((n, trace), dtype=torch.float32, device=dev)
    adc = torch.empty((n, trace), dtype=torch.int16, device=dev)
    scale = (0.1755 * (1.0 + 0.02 * (2 * torch.rand(n, generator=g, device=dev) - 1))).float()
    offset = torch.round(-240.0 + 20.0 * (2 * torch.rand(n, generator=g, device=dev) - 1)).float()
    idx = torch.arange(trace, device=dev)[None, :]
    ev = (trace + 39) // 40
    for r0 in range(0, n, chunk):
        m = min(chunk, n - r0)

        def draw(lo, hi):
            return torch.randint(lo, hi + 1, (m, 1), generator=g, device=dev)

        b0 = draw(0, 400)
        b1 = b0 + draw(2000, 6000)
        b2 = b1 + draw(400, 3000)
        level = torch.randn((m, ev), generator=g, device=dev).repeat_interleave(40, dim=1)[:, :trace]
        noise = torch.randn((m, trace), generator=g, device=dev)
        x = torch.where(idx < b0, 220.0 + 3.0 * noise,
                        torch.where(idx < b1, 80.0 + 12.0 * level + 2.5 * noise,
                                    torch.where(idx < b2, 108.0 + 1.2 * noise, 95.0 + 15.0 * level + 3.0 * noise)))
        sc, of = scale[r0:r0 + m, None], offset[r0:r0 + m, None]
        q = torch.clamp(torch.round(x / sc - of), -32768, 32767).to(torch.int16)
        adc[r0:r0 + m] = q
        sig[r0:r0 + m] = (q.float() + of) * sc
        del level, noise, x, q
    return sig, adc, offset, scale


def _restate(args):
    from helpers import detect_rule as dr

    seed, first, n, trace = args
    rows = [dr.synth_trace(seed, first + i, trace)[0] for i in range(n)]
    t0 = time.perf_counter()
    dr.detect_rows(rows, dr.DEFAULT)
    return time.perf_counter() - t0


def numpy_rate(workers, reads_per_worker, trace):
    """reads/s of the NumPy restatement with `workers` processes at work at once (wall clock of the slowest worker's rule time)"""
    import multiprocessing as mp

    with mp.get_context("fork").Pool(workers) as pool:
        times = pool.map(_restate, [(99, w * reads_per_worker, reads_per_worker, trace) for w in range(workers)])
    return workers * reads_per_worker / max(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--trace", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=7, help="timed alternations after two warm-up rounds (at least 5)")
    ap.add_argument("--numpy-workers", type=int, default=16)
    ap.add_argument("--numpy-reads", type=int, default=256, help="reads each worker of the NumPy restatement takes")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    np_rate, np_times = numpy_rate(args.numpy_workers, args.numpy_reads, args.trace)     # (before the GPU is opened: forked workers, no device in them)

    import numpy as np
    import torch

    from warpdemux_amd import _lib, sig_proc
    from warpdemux_amd.engine import AdcShard, DemuxEngine

    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_detect.py measures on an MI355X: no device is visible")
    reps = max(5, args.reps)
    n, trace = args.reads, args.trace
    eng = DemuxEngine(np.zeros((2, 25)), 15, 0.1)
    params = sig_proc.DetectParams(max_obs_trace=trace)
    sig, adc, offset, scale = generate(torch, n, trace, eng.tdev)
    row_len = torch.full((n,), trace, dtype=torch.int32, device=eng.tdev)
    shard = AdcShard(adc, row_len, offset, scale)
    torch.cuda.synchronize()

    paths = {"float32": lambda: eng.detect(sig, params=params, want_info=True),
             "int16": lambda: eng.detect(shard, params=params, want_info=True)}
    res = {}
    for _ in range(2):                                   # warm-up: the code objects, torch's allocator
        for k, f in paths.items():
            res[k] = f()
    torch.cuda.synchronize()
    fields = ("a_start", "a_end", "ok", "code", "info")
    identical = all(bool(torch.equal(getattr(res["float32"], f), getattr(res["int16"], f))) for f in fields)
    identical = identical and bool(torch.equal(res["float32"].gain.view(torch.int64), res["int16"].gain.view(torch.int64)))
    codes = torch.bincount(res["float32"].code, minlength=5).tolist()

    ms = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))

    kernel_ms = {}
    for k, f in paths.items():                           # the kernel alone: the library's event brackets, a run of their own
        eng.kernel_time_reset()
        eng.kernel_timing(True)
        f()
        torch.cuda.synchronize()
        kernel_ms[k] = eng.kernel_time(_lib.K_DETECT)[0]
        eng.kernel_timing(False)

    # what binds: the same rows with ONE candidate in steps 3 and 4 (max_obs_adapter = min_obs_adapter) -- the load, the
    # quantisation and step 2 remain; the difference to kernel_ms is the candidates' arithmetic
    one = sig_proc.DetectParams(max_obs_trace=trace, max_obs_adapter=params.min_obs_adapter)
    one_paths = {"float32": lambda: eng.detect(sig, params=one), "int16": lambda: eng.detect(shard, params=one)}
    one_ms = {}
    for k, f in one_paths.items():
        f()
        torch.cuda.synchronize()
        eng.kernel_time_reset()
        eng.kernel_timing(True)
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        one_ms[k] = eng.kernel_time(_lib.K_DETECT)[0] / 3
        eng.kernel_timing(False)

    def summary(k, bytes_per_sample):
        v = ms[k]
        med = statistics.median(v)
        floor_ms = n * trace * bytes_per_sample / HBM_PEAK_BYTES_PER_S * 1e3
        return {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 3) for x in v], "method_reads_per_s": n / med * 1e3,
                "kernel_ms": kernel_ms[k], "kernel_reads_per_s": n / kernel_ms[k] * 1e3 if kernel_ms[k] > 0 else None, "input_bytes": n * trace * bytes_per_sample, "hbm_floor_ms": floor_ms,
                "fraction_of_hbm_floor": floor_ms / kernel_ms[k] if kernel_ms[k] > 0 else None,
                "kernel_ms_one_candidate": one_ms[k], "candidates_ms": kernel_ms[k] - one_ms[k]}

    out = {
        "tool": "tools/bench_detect.py", "device": torch.cuda.get_device_name(0), "reads": n, "trace_samples": trace, "reps": reps,
        "warmup_rounds": 2, "params": {k: getattr(params, k) for k in params.__dataclass_fields__}, "results_identical": identical,
        "codes": dict(zip(("ok", "short", "no_start", "no_room", "no_polya"), codes)),
        "float32": summary("float32", 4), "int16": summary("int16", 2),
        "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
        "numpy_restatement": {"workers": args.numpy_workers, "reads_per_worker": args.numpy_reads, "reads_per_s": np_rate,
                              "worker_seconds": [round(t, 3) for t in np_times]},
        "note": "synthetic traces; the engine's own rule; parity with ADAPTed unpinned; accuracy on real reads unmeasured",
    }
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if not identical:
        raise SystemExit("the int16 path and the float32 path disagree")


if __name__ == "__main__":
    main()
