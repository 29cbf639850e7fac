"""Run by tests/test_gpu_marshal.py in a FRESH interpreter (the parent of a Feeder must not have touched the GPU): a `success`
array of the wrong shape is refused in Python by `Feeder.fingerprint_batch` and `Feeder.demux_batch`, and the ring then serves
the next well-formed minibatch.  Writes what was refused, the ring's free slots after the refusals and the results of the
well-formed calls to the .npz named on the command line.  `inputs()` is the minibatch of that test."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

N, STRIDE, WINDOW_SAMPLES, PADDING, K, N_REFS = 8, 1024, 600, 100, 25, 4
SEG = dict(padding=PADDING, min_obs_per_base=4, running_stat_width=8, num_events=35, barcode_num_events=K)
I_DEAD = 5      # the one read whose detection failed: a flag that slips by one row shows in two statuses


def inputs(seed=11):
    """dict: rows (N, STRIDE) float32, a_s / a_e int32 (windows of WINDOW_SAMPLES samples with the padding, at scattered
    starts), ok uint8 (0 at I_DEAD), refs (N_REFS, K) float64"""
    rng = np.random.default_rng(seed)
    rows = np.empty((N, STRIDE), dtype=np.float32)
    for r in range(N):
        lv = rng.normal(0, 1, 160) * 12.0 + 85.0
        rows[r] = (np.repeat(lv, rng.integers(7, 13, lv.size))[:STRIDE] + rng.normal(0, 1.5, STRIDE)).astype(np.float32)
    a_s = (PADDING + rng.integers(0, STRIDE - WINDOW_SAMPLES, N)).astype(np.int32)
    a_e = (a_s + WINDOW_SAMPLES - 2 * PADDING).astype(np.int32)
    ok = np.ones(N, dtype=np.uint8)
    ok[I_DEAD] = 0
    return dict(rows=rows, a_s=a_s, a_e=a_e, ok=ok, refs=rng.normal(size=(N_REFS, K)))


def bad_success():
    """one entry short, and one column too many"""
    return np.ones(N - 1, dtype=np.uint8), np.ones((N, 2), dtype=np.uint8)


if __name__ == "__main__":
    from warpdemux_amd import sig_proc
    from warpdemux_amd.feeder import Feeder

    b = inputs()
    refused = []
    with Feeder(b["refs"], 15, 0.1, sig_proc.SegParams(**SEG), max_reads=N, stride=STRIDE, n_slots=4) as f:
        for call in (f.fingerprint_batch, f.demux_batch):
            for bad in bad_success():
                try:
                    call(b["rows"], b["a_s"], b["a_e"], success=bad)
                    refused.append(False)
                except ValueError:
                    refused.append(True)
        free = f.stats()["free_slots"]
        fb = f.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], success=b["ok"])
        db = f.demux_batch(b["rows"], b["a_s"], b["a_e"], success=b["ok"])
    np.savez(sys.argv[1], refused=refused, free_slots=free, fpt=fb.fpt, dwell=fb.dwell, stats=fb.stats, status=fb.status,
             demux_status=db.status, call=db.call, dist=db.dist)
