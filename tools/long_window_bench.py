#!/usr/bin/env python3
"""Fingerprint-stage throughput by adapter-window length (device-resident minibatch layout), for one parameter triple:
which kernel a window reaches and what it costs there.   python tools/long_window_bench.py [E d W] [n_reads]

    python tools/long_window_bench.py --long [n_reads]

the long form of the exact kernel (``long_windows=True``: windows beyond 16 384 samples, fingerprint_long_kernel) at 20 000 and
65 536 samples for the three shipped triples, beside the CPU oracle on one core of this machine; one JSON line per row.

    python tools/long_window_bench.py --refine [n_reads]

the same for the consensus-refinement branch (fingerprint_long_refine_kernel): tRNA parameters, reads that carry the consensus
of fixture g8 (random leader | consensus | 30 barcode levels, dwell times scaled to the window)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from warpdemux_amd import sig_proc  # noqa: E402
from warpdemux_amd.engine import DemuxEngine  # noqa: E402



def long_mode(n):
    import json

    from oracle import wdx_oracle as orc

    rng = np.random.default_rng(1)
    for name, (E, d, W) in (("rna004", (110, 6, 12)), ("rna002", (110, 15, 30)), ("trna", (120, 9, 18))):
        kw = dict(padding=0, num_events=E, min_obs_per_base=d, running_stat_width=W, barcode_num_events=25)
        eng = DemuxEngine(np.zeros((4, 25)), 15, 0.1, sig_proc.SegParams(**kw), long_windows=True)
        for ln in (20000, 65536):
            dw = max(12, ln // 135)
            base = (np.repeat(rng.normal(80, 15, (16, ln // dw + 1)), dw, axis=1)[:, :ln] + rng.normal(0, 2, (16, ln))).astype(np.float32)
            mb = torch.from_numpy(np.tile(base, (n // 16, 1))).cuda()
            a_s = torch.zeros(n, dtype=torch.int32, device="cuda")
            a_e = torch.full((n,), ln, dtype=torch.int32, device="cuda")
            for _ in range(2):
                out = eng.fingerprint(mb, a_s, a_e, stride=ln, max_len=ln)
            torch.cuda.synchronize()
            reps = 3
            t0 = time.perf_counter()
            for _ in range(reps):
                out = eng.fingerprint(mb, a_s, a_e, stride=ln, max_len=ln)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / reps
            t0 = time.perf_counter()
            ref = orc.fingerprint_batch(base, np.zeros(16, np.int32), np.full(16, ln, np.int32), orc.SegParams(**kw))
            dt_cpu = (time.perf_counter() - t0) / 16
            same = bool(np.array_equal(out[0][:16].cpu().numpy(), ref[0], equal_nan=True))
            print(json.dumps(dict(triple=name, window=ln, n_reads=n, gpu_reads_per_s=round(n / dt, 1), gpu_ms_per_call=round(dt * 1e3, 3),
                                  ok=int((out[3] == 0).sum().item()), oracle_reads_per_s_one_core=round(1.0 / dt_cpu, 1),
                                  bit_identical_to_oracle=same)), flush=True)
        eng.ctx.close()


def refine_mode(n):
    import json

    from oracle import wdx_oracle as orc

    q = np.load(os.path.join(ROOT, "tests", "golden", "g8_refine.npz"))["consensus"]
    rng = np.random.default_rng(2)
    seg = dict(padding=0, num_events=120, min_obs_per_base=9, running_stat_width=18, barcode_num_events=25)
    hr, orr = sig_proc.RefineParams(query=q), orc.RefineParams(query=q)
    eng = DemuxEngine(np.zeros((4, 25)), 15, 0.1, sig_proc.SegParams(clip_bounds="float32", **seg), long_windows=True)
    for ln in (20000, 65536):
        base = np.empty((16, ln), dtype=np.float32)
        for i in range(16):
            lv = np.concatenate([rng.normal(0, 1, int(rng.integers(4, 14))), q, rng.normal(0, 1, 30)]) * 12.0 + 85.0
            dw = rng.integers(14, 60, lv.size)
            dw = np.maximum(dw * ln // int(dw.sum()), 1)
            dw[0] += ln - int(dw.sum())
            base[i] = np.repeat(lv, dw) + rng.normal(0, 1.5, ln)
        mb = torch.from_numpy(np.tile(base, (n // 16, 1))).cuda()
        a_s = torch.zeros(n, dtype=torch.int32, device="cuda")
        a_e = torch.full((n,), ln, dtype=torch.int32, device="cuda")
        for _ in range(2):
            out = eng.fingerprint_refine(mb, a_s, a_e, hr, stride=ln, max_len=ln)
        torch.cuda.synchronize()
        reps = 3
        t0 = time.perf_counter()
        for _ in range(reps):
            out = eng.fingerprint_refine(mb, a_s, a_e, hr, stride=ln, max_len=ln)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        t0 = time.perf_counter()
        ref = orc.fingerprint_refine_batch(base, np.zeros(16, np.int32), np.full(16, ln, np.int32), orc.SegParams(**seg), orr)
        dt_cpu = (time.perf_counter() - t0) / 16
        same = bool(np.array_equal(out[0][:16].cpu().numpy(), ref[0], equal_nan=True) and
                    np.array_equal(out[4][:16].cpu().numpy(), ref[4]) and np.array_equal(out[3][:16].cpu().numpy(), ref[3]))
        print(json.dumps(dict(branch="refine", triple="trna", window=ln, n_reads=n, gpu_reads_per_s=round(n / dt, 1),
                              gpu_ms_per_call=round(dt * 1e3, 3), ok=int((out[4] == 0).sum().item()),
                              outliers=int((out[4] == 6).sum().item()), oracle_reads_per_s_one_core=round(1.0 / dt_cpu, 1),
                              bit_identical_to_oracle=same)), flush=True)
    eng.ctx.close()


if len(sys.argv) > 1 and sys.argv[1] == "--refine":
    refine_mode(int(sys.argv[2]) if len(sys.argv) > 2 else 256)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "--long":
    long_mode(int(sys.argv[2]) if len(sys.argv) > 2 else 256)
    sys.exit(0)
E, d, W = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (110, 15, 30)
n = int(sys.argv[4]) if len(sys.argv) > 4 else 8192
rng = np.random.default_rng(1)
params = sig_proc.SegParams(padding=0, num_events=E, min_obs_per_base=d, running_stat_width=W, barcode_num_events=25)
eng = DemuxEngine(np.zeros((4, 25)), 15, 0.1, params)
print(f"triple ({E},{d},{W}), {n} reads per length")
for ln in (4600, 6000, 7500, 8192, 9000, 11200, 12000, 15200):
    dw = max(12, ln // 135)
    base = (np.repeat(rng.normal(80, 15, (64, ln // dw + 1)), dw, axis=1)[:, :ln] + rng.normal(0, 2, (64, ln))).astype(np.float32)
    mb = torch.from_numpy(np.tile(base, (n // 64, 1))).cuda()
    a_s = torch.zeros(n, dtype=torch.int32, device="cuda")
    a_e = torch.full((n,), ln, dtype=torch.int32, device="cuda")
    for _ in range(2):
        out = eng.fingerprint(mb, a_s, a_e, stride=ln, max_len=ln)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        out = eng.fingerprint(mb, a_s, a_e, stride=ln, max_len=ln)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    ok = int((out[3] == 0).sum().item())
    print(f"  window {ln:6d}: {n / dt / 1e6:7.3f} M reads/s  ({dt * 1e3:8.2f} ms, {ok} ok; {n * ln * 4 / dt / 1e9:7.1f} GB/s of samples)")
