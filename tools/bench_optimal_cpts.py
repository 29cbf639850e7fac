#!/usr/bin/env python3
"""Rate of the device-resident consensus-refinement flow (DemuxEngine.fingerprint_refine: wdx_fingerprint_refine_dev) on
synthetic tRNA-shaped reads (120 events, d = 9, W = 18, 25 barcode events) with WDX_OPT_REFINE_OPTIMAL_CPTS on, beside the
same flow with the option off on the same tree.  Wall time between device synchronisations of whole calls, and the HIP-event
time of the fingerprint chain (WDX_K_FINGERPRINT) and of fingerprint_refine_optimal_kernel alone (WDX_K_REFINE_OPTIMAL).

    python tools/bench_optimal_cpts.py [n_reads] [reps] [out.json]      # one JSON record -> profiles/optimal_cpts.json
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from warpdemux_amd import _lib, sig_proc  # noqa: E402
from warpdemux_amd.engine import DemuxEngine  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
consensus = np.load(os.path.join(ROOT, "tests", "golden", "g8_refine.npz"))["consensus"]
rng = np.random.default_rng(3)
DISTINCT = min(n, 2048)      # distinct reads, tiled to n (the kernels do not know)
rows, orig = [], []
for i in range(DISTINCT):
    lv = np.concatenate([rng.normal(0, 1, int(rng.integers(2, 16))), consensus, rng.normal(0, 1, 30)]) * 12.0 + 85.0
    dw = rng.integers(12, 60, lv.size)
    x = (np.repeat(lv, dw) + rng.normal(0, 1.5, int(dw.sum()))).astype(np.float32)
    orig.append(x.size)
    rows.append(np.concatenate([x, np.zeros(-x.size % 4, np.float32)]))   # (rows start on 16-byte boundaries)
sizes = np.array([r.size for r in rows])
reps_of = -(-n // DISTINCT)
flat = np.tile(np.concatenate(rows), reps_of)
lens = np.tile(sizes, reps_of)[:n]
off = np.concatenate([[0], np.cumsum(np.tile(sizes, reps_of))]).astype(np.int64)[: n + 1]

import torch  # noqa: E402

seg = sig_proc.SegParams(min_obs_per_base=9, running_stat_width=18, num_events=120, barcode_num_events=25)
eng = DemuxEngine(np.zeros((2, 25)), 15, 0.1, seg)
L = _lib.load()
d_sig, d_off = torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()
d_as = torch.full((n,), 100, dtype=torch.int32, device="cuda")
d_ae = torch.from_numpy((np.tile(np.array(orig), reps_of)[:n] - 100).astype(np.int32)).cuda()
max_len = int(sizes.max())


def run(optimal):
    ref = sig_proc.RefineParams(query=consensus, barcode_segm_events=25, barcode_keep_events=25, optimal_cpts=optimal)
    call = lambda: eng.fingerprint_refine(d_sig, d_as, d_ae, ref, offsets=d_off, max_len=max_len)   # noqa: E731
    out = call()
    torch.cuda.synchronize()
    _lib.check(L.wdx_kernel_time_reset(eng.ctx.handle))
    _lib.check(L.wdx_kernel_timing(eng.ctx.handle, 1))
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    _lib.check(L.wdx_kernel_timing(eng.ctx.handle, 0))
    ms = {}
    for name, kid in (("fingerprint_chain", _lib.K_FINGERPRINT), ("refine_optimal_kernel", _lib.K_REFINE_OPTIMAL)):
        t, k = C.c_double(0), C.c_int64(0)
        _lib.check(L.wdx_kernel_time(eng.ctx.handle, kid, C.byref(t), C.byref(k)))
        ms[name] = round(t.value / reps, 3)
    st = out[4].cpu().numpy()
    wall = float(np.median(walls))
    return dict(reads_per_s=round(n / wall), wall_ms_median=round(wall * 1e3, 3), wall_ms_all=[round(w * 1e3, 3) for w in walls],
                kernel_ms_per_call=ms, status_histogram={int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))})


rec = dict(what="wdx_fingerprint_refine_dev, packed float32 reads resident on the device", n_reads=n, reps=reps,
           mean_window_samples=round(float(lens.mean())), triple=[120, 9, 18], barcode_num_events=[25, 25],
           option_off=run(False), option_on=run(True))
rec["option_off_again"] = run(False)
usage = os.path.join(ROOT, "profiles", "optimal_cpts_resource_usage.txt")
if os.path.exists(usage):
    rec["resource_usage"] = [ln.strip() for ln in open(usage) if ln.strip()]
eng.close()
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "optimal_cpts.json")
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
