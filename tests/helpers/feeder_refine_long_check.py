"""Run by tests/test_gpu_long_refine.py in a FRESH interpreter (the parent of a Feeder must not have touched the GPU): the 12
reads of tests/helpers/refine_long_inputs.py -- adapter windows up to 65 536 samples -- through one forked worker each of a
fingerprint-only ``Feeder(refine=..., long_windows=True)`` on float32 rows and of one on int16 rows.  Writes status / fpt /
dwell / stats / refine_idx of both to the .npz named on the command line."""
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from helpers import refine_inputs as ri  # noqa: E402
from helpers import refine_long_inputs as rl  # noqa: E402
from warpdemux_amd import sig_proc  # noqa: E402
from warpdemux_amd.feeder import Feeder  # noqa: E402

FEEDERS = {}     # inherited by the forked worker


def _worker(kind, out):
    b, f = rl.ways_batch(), FEEDERS[kind]
    if kind == "i16":
        fb = f.fingerprint_batch_adc(b["adc"], b["row_len"], b["offset"], b["scale"], b["a_s"], b["a_e"], success=b["ok"])
    else:
        fb = f.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], success=b["ok"])
    np.savez(out, status=fb.status, fpt=fb.fpt, dwell=fb.dwell, stats=fb.stats, refine_idx=fb.refine_idx)


if __name__ == "__main__":
    b = rl.ways_batch()
    params = sig_proc.SegParams(barcode_num_events=rl.K, clip_bounds="float32", **ri.SEG)
    refine = sig_proc.RefineParams(query=ri.consensus(), **ri.REF)
    parts = {}
    for kind in ("f32", "i16"):
        with Feeder(params=params, refine=refine, max_reads=12, stride=b["rows"].shape[1], n_slots=2, adc=kind == "i16",
                    long_windows=True) as f:
            FEEDERS[kind] = f
            part = sys.argv[1] + "." + kind + ".npz"
            w = mp.get_context("fork").Process(target=_worker, args=(kind, part))
            w.start()
            w.join(240)
            if w.is_alive():
                w.terminate()
                sys.exit("the feeder worker did not finish")
            if w.exitcode:
                sys.exit(w.exitcode)
            parts[kind] = dict(np.load(part))
        del FEEDERS[kind]
    np.savez(sys.argv[1], **{f"{kind}_{name}": a for kind, d in parts.items() for name, a in d.items()})
