"""Run by tests/test_gpu_window_edges.py in a FRESH interpreter (the parent of a Feeder must not have touched the GPU): the
batch of tests/helpers/window_inputs.py through a feeder worker's packing, from an array with no slack behind its last
row.  Writes status / fpt / call to the .npz named on the command line."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from helpers import window_inputs as wi  # noqa: E402
from warpdemux_amd import sig_proc  # noqa: E402
from warpdemux_amd.feeder import Feeder  # noqa: E402

if __name__ == "__main__":
    b = wi.batch()
    refs = wi.oracle(b)[2]
    rows = np.ascontiguousarray(b["rows"])             # exactly N * STRIDE floats: the last row ends the buffer
    with Feeder(refs, 15, 0.1, sig_proc.SegParams(**wi.SEG), max_reads=wi.N, stride=wi.STRIDE, n_slots=2) as f:
        fb = f.fingerprint_batch(rows, b["a_s"], b["a_e"], success=b["ok"])
        db = f.demux_batch(rows, b["a_s"], b["a_e"], success=b["ok"], want_dist=False)
    np.savez(sys.argv[1], status=fb.status, fpt=fb.fpt, call=db.call, demux_status=db.status)
