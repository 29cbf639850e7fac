"""Run by tests/test_gpu_wide_dtw.py in a FRESH interpreter (the parent of a Feeder must not have touched the GPU): the first
64 reads of tests/helpers/wide_inputs.synth_batch through one forked feeder worker of a ``Feeder(window=None,
wide_dtw=True)`` on 110-point references.  Writes status / call / dist to the .npz named on the command line and, beside it
(``<name>.route.json``), what the SERVING context says when `_serve` closes it: its WDX_OPT_WIDE_DTW flag and the DTW kernel its
last dispatch took (wdx_dtw_last_launch) -- the serving process is forked from this one, so a wrapper around
`_lib.Context.close` installed here runs there."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from helpers import wide_inputs as wi  # noqa: E402
from warpdemux_amd import _lib, sig_proc  # noqa: E402
from warpdemux_amd.feeder import Feeder  # noqa: E402


def _report_route_on_close(path):
    """`Context.close` of this process and its forks first writes the context's option flag and last DTW route to `path`.
    Only the forked `_serve` owns a context: neither this process nor the worker creates one."""
    close = _lib.Context.close

    def close_and_report(self):
        if self._h is not None and self.pid == os.getpid():
            i = self.dtw_last_launch()
            with open(path, "w") as fh:
                json.dump({"wide_dtw": bool(self.wide_dtw), "family": _lib.DTW_FAMILY_NAMES[i.family],
                           "layout": _lib.DTW_LAYOUT_NAMES[i.layout], "window": int(i.window), "launches": int(i.launches)}, fh)
        close(self)

    _lib.Context.close = close_and_report


def _worker(f, b, out):
    db = f.demux_batch(b["rows"][:64], b["a_s"][:64], b["a_e"][:64], success=b["ok"][:64], want_dist=True)
    np.savez(out, status=db.status, call=db.call, dist=db.dist)


if __name__ == "__main__":
    import multiprocessing as mp

    b = wi.synth_batch()
    params = sig_proc.SegParams(barcode_num_events=110, padding=b["padding"])
    _report_route_on_close(sys.argv[1] + ".route.json")
    with Feeder(wi.host_refs(), None, 0.1, params, max_reads=64, stride=b["rows"].shape[1], n_slots=2, wide_dtw=True) as f:
        w = mp.get_context("fork").Process(target=_worker, args=(f, b, sys.argv[1]))
        w.start()
        w.join(240)
        if w.is_alive():
            w.terminate()
            sys.exit("the feeder worker did not finish")
        sys.exit(w.exitcode)
