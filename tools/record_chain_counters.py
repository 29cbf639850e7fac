#!/usr/bin/env python
"""Which list each launch of the fingerprint chain takes and feeds, seen from outside: the eight counters a call leaves at the
front of its workspace and the launches it reports, for nine cases of 4 096 reads.  Uses the public engine only, so it runs on
any tree: run ONCE, on the commit BEFORE a change of the launch code, it writes tests/golden/fp_chain_counters.json, which
tests/test_gpu_fp_chain_counters.py then holds the changed tree to.

  python tools/record_chain_counters.py            print the nine records
  python tools/record_chain_counters.py --write    ... and write the golden file

The recording is refused unless each of slow, big0, big1, retry and big2 is non-zero in some case and back is non-zero in the
refinement case (change the inputs, not the condition).

Two counters are not functions of the reads alone.  Where a list is longer than the grid of its one-workgroup-per-entry kernel
(1 024 entries at 4 096 reads), its first entries take that kernel and the rest the striding 8192-sample kernel, and WHICH reads
come first is the order in which workgroups won the list's atomic counter: the two kernels have other capacities, so a few reads
are declined (slow) or redone (retry) by one and not by the other.  The windows cut to 5 120, 6 144 and 8 192 samples are such cases.
So every case is recorded --repeats times, other cases run in between and other work beside it, and the file keeps each counter's lowest and highest
value; the test asks for the exact value where the two agree, and otherwise for the recorded range widened by itself once."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import framed as fr  # noqa: E402  (where the counters lie inside d_work)
from helpers import refine_inputs as ri  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fp_chain_counters.json")
N, K, CHAIN_MIN = 4096, 25, 1024
GRID = 1024   # workgroups of the one-workgroup-per-entry list kernels at N reads: max(1024, N / 4)
# name -> (num_events, min_obs_per_base, running_stat_width, longest window, refines)
CASES = {
    "W12_d6_max4096": (110, 6, 12, 4096, False), "W12_d6_max5120": (110, 6, 12, 5120, False),
    "W12_d6_max6144": (110, 6, 12, 6144, False), "W12_d6_max8192": (110, 6, 12, 8192, False),
    "W12_d6_max12288": (110, 6, 12, 12288, False), "W12_d6_max16384": (110, 6, 12, 16384, False),
    "W30_d15": (110, 15, 30, 8192, False), "refine_W18_d9": (120, 9, 18, 8192, True), "W13": (110, 6, 13, 8192, False),
}


def _synthetic(eng, cut, padding):
    """4 096 synthetic reads in HBM, the adapter windows cut to `cut` samples"""
    import torch

    from warpdemux_amd import synth

    sig, off, a_s, a_e, _bc, _longest = eng.synth_packed(synth.SynthSpec(n_barcodes=10, dwell_scale=2.5), 0, N)
    a_e = torch.minimum(a_e, torch.full_like(a_e, cut - padding))
    return sig, off, a_s, a_e, None


def _long_tail_row(seed):
    """(tests/test_gpu_buffer_bounds.py) a read that carries the consensus and whose 30 levels behind it dwell 75 .. 100 samples
    each: its barcode tail is longer than the tail kernel takes, so it comes back on the back list"""
    q, rng = ri.consensus(), np.random.default_rng(seed)
    lv = np.concatenate([rng.normal(0, 1, 4), q, rng.normal(0, 1, 30)]) * 12.0 + 85.0
    dw = np.concatenate([rng.integers(12, 40, 4 + q.size), rng.integers(75, 100, 30)])
    return (np.repeat(lv, dw) + rng.normal(0, 1.5, int(dw.sum()))).astype(np.float32)


def _consensus_reads():
    """the 96 reads of tests/helpers/refine_inputs.py drawn 4 096 times, every 64th a read with a long barcode tail"""
    import torch

    b = ri.batch(1)
    idx = np.concatenate([np.arange(96), np.random.default_rng(1).integers(0, 96, N - 96)])
    rows, a_s, a_e, ok = [], b["a_s"][idx].copy(), b["a_e"][idx].copy(), b["ok"][idx].copy()
    for r in range(N):
        if r % 64 == 17:
            x = _long_tail_row(r)
            a_s[r], a_e[r], ok[r] = ri.PADDING, x.size - ri.PADDING, 1
        else:
            x = b["rows"][idx[r]]   # (with its NaN tail: one read's window reaches into it)
        rows.append(np.ascontiguousarray(x, dtype=np.float32))
    off = np.concatenate([[0], np.cumsum([x.size for x in rows])]).astype(np.int64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return dev(np.concatenate(rows)), dev(off), dev(a_s.astype(np.int32)), dev(a_e.astype(np.int32)), dev(ok.astype(np.uint8))


def record(name):
    """the counters and the reported launches of one case"""
    import torch

    from warpdemux_amd import _lib, sig_proc
    from warpdemux_amd.engine import DemuxEngine

    E, d, W, cut, refines = CASES[name]
    params = sig_proc.SegParams(barcode_num_events=K, padding=ri.PADDING, min_obs_per_base=d, running_stat_width=W, num_events=E)
    refs = np.ascontiguousarray(np.random.default_rng(5).normal(size=(10, K)))
    eng = DemuxEngine(refs, 15, 0.1, params)
    try:
        eng.ctx.set_option(_lib.OPT_FAST_CHAIN_MIN_READS, CHAIN_MIN)
        sig, off, a_s, a_e, ok = _consensus_reads() if refines else _synthetic(eng, cut, params.padding)
        eng.kernel_timing(True)
        eng.kernel_time_reset()
        if refines:
            hr = sig_proc.RefineParams(query=ri.consensus(), **ri.REF)
            eng.demux_refine(sig, a_s, a_e, hr, offsets=off, max_len=cut, ok=ok)
            work = eng._refine_work
        else:
            eng.demux(sig, a_s, a_e, offsets=off, max_len=cut, ok=ok)
            work = eng._work
        torch.cuda.synchronize()
        at = fr.work_pieces(N, K)["fp_ws"]
        raw = work[at:at + 4 * fr.N_COUNTERS].cpu().numpy().view(np.uint32)
        out = dict(zip(fr.COUNTER_NAMES, (int(v) for v in raw)))
        out["n_launches"] = int(eng.kernel_time(_lib.K_FINGERPRINT)[1])
        out["n_launches_main"] = int(eng.kernel_time(_lib.K_FINGERPRINT_MAIN)[1])
        return out
    finally:
        eng.close()


def _busy(i):
    """a product of two matrices on a side stream, of another size each time: which workgroup of a launch starts first -- and
    so the order of a list's entries -- depends on what else the CUs hold"""
    import torch

    if i % 3 == 0:
        return None
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = torch.ones((1024 * (1 + i % 5), 2048), device="cuda")
        return [a @ a.T for _ in range(1 + i % 4)]


def acceptable(rec):
    """[] or what the recording (case -> counter -> [lowest, highest]) lacks"""
    lacks = [c for c in ("slow", "big0", "big1", "retry", "big2") if not any(r[c][0] for r in rec.values())]
    if not rec["refine_W18_d9"]["back"][0]:
        lacks.append("back (refinement case)")
    return lacks


def allowed(lo_hi):
    """the values a counter recorded as [lowest, highest] may take: that range widened by its own width either side"""
    lo, hi = lo_hi
    return range(max(lo - (hi - lo), 0), hi + (hi - lo) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--repeats", type=int, default=60)
    args = ap.parse_args()
    names, rec = list(CASES), {}
    for i in range(args.repeats):
        for name in np.random.default_rng(i).permutation(names):   # (another order each time: other leftovers, other timing)
            busy = _busy(i)   # (... and, two times in three, other work on the CUs while the call's first kernels start)
            r = record(name)
            del busy
            for c, v in r.items():
                lo_hi = rec.setdefault(name, {}).setdefault(c, [v, v])
                lo_hi[0], lo_hi[1] = min(lo_hi[0], v), max(lo_hi[1], v)
    for name in names:
        print(name, json.dumps(rec[name]))
    lacks = acceptable(rec)
    if lacks:
        print("not acceptable: never non-zero:", ", ".join(lacks))
        return 1
    if args.write:
        if os.path.exists(args.out):   # (a further recording widens what the file holds)
            with open(args.out) as fh:
                old = json.load(fh)
            rec = {n: {c: [min(v[0], old[n][c][0]), max(v[1], old[n][c][1])] for c, v in r.items()} for n, r in rec.items()}
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
