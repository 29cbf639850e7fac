"""Run by tests/test_gpu_optimal_cpts.py in a FRESH interpreter (the parent of a Feeder must not have touched the GPU):
the nine reads of fixture g14 that share one parameter set, as one minibatch through Feeder(refine=RefineParams(...,
optimal_cpts=True)).  Every output bit for bit against the fixture.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from helpers import optimal_inputs as oi  # noqa: E402
from warpdemux_amd.feeder import Feeder  # noqa: E402

if __name__ == "__main__":
    mb = oi.g14_minibatch()
    with Feeder(refine=mb["refine"], params=mb["params"], max_reads=16, stride=mb["rows"].shape[1], n_slots=2) as f:
        fb = f.fingerprint_batch(mb["rows"], mb["a_s"], mb["a_e"])
    got = dict(status=fb.status, fpt=fb.fpt, dwell=fb.dwell, stats=fb.stats, refine_idx=fb.refine_idx)
    print(json.dumps({k: oi.same(got[k], mb[k]) for k in got}))
