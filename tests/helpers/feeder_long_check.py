"""Run by tests/test_gpu_long_windows.py in a FRESH interpreter (the parent of a Feeder must not have touched the GPU): the
12 reads of tests/helpers/long_inputs.py -- adapter windows up to 65 536 samples -- through one forked feeder worker of a
``Feeder(long_windows=True)``.  Writes status / fpt / call to the .npz named on the command line."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from helpers import long_inputs as li  # noqa: E402
from oracle import wdx_oracle as orc  # noqa: E402
from warpdemux_amd import sig_proc  # noqa: E402
from warpdemux_amd.feeder import Feeder  # noqa: E402


def _worker(f, b, out):
    fb = f.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], success=b["ok"])
    db = f.demux_batch(b["rows"], b["a_s"], b["a_e"], success=b["ok"], want_dist=False)
    np.savez(out, status=fb.status, fpt=fb.fpt, call=db.call, demux_status=db.status)


if __name__ == "__main__":
    import multiprocessing as mp

    b = li.ways_batch()
    want = orc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], orc.SegParams(clip_bounds_f64=False, **li.WAYS_SEG), ok=b["ok"])
    good = np.flatnonzero(want[3] == 0)
    refs = np.ascontiguousarray(np.concatenate([want[0][good], want[0][good[:1]] + 0.25])[:10])
    params = sig_proc.SegParams(clip_bounds="float32", **li.WAYS_SEG)
    with Feeder(refs, 15, 0.1, params, max_reads=12, stride=b["rows"].shape[1], n_slots=2, long_windows=True) as f:
        w = mp.get_context("fork").Process(target=_worker, args=(f, b, sys.argv[1]))
        w.start()
        w.join(240)
        if w.is_alive():
            w.terminate()
            sys.exit("the feeder worker did not finish")
        sys.exit(w.exitcode)
