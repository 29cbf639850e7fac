"""The float32 doors' shared check on the device side of things: a `success` array of the wrong shape is refused in Python --
nothing of it reaches the library -- by `MinibatchPipeline.submit`, `Feeder.fingerprint_batch` and `Feeder.demux_batch`, and
the slot and the ring then serve the next well-formed minibatch with the bits of the blocking calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import feeder_success_check as fsc
from warpdemux_amd import pipeline, sig_proc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_a_refused_success_array_costs_neither_the_slot_nor_the_ring(tmp_path):
    b = fsc.inputs()
    rows, a_s, a_e, ok = b["rows"], b["a_s"], b["a_e"], b["ok"]
    params = sig_proc.SegParams(**fsc.SEG)
    sig_proc.set_references(b["refs"], 15, 0.1)
    want = sig_proc.demux_batch(rows, a_s, a_e, params, success=ok, want_dist=True, want_fpt=True)
    want_fb = sig_proc.fingerprint_batch(rows, a_s, a_e, params, success=ok)
    assert want.status[fsc.I_DEAD] == 1 and (want.status == 0).sum() == fsc.N - 1      # (what the CPU oracle gives too)
    assert _same(want.status, want_fb.status) and _same(want.fpt, want_fb.fpt)

    pipe = pipeline.MinibatchPipeline(b["refs"], 15, 0.1, params, n_slots=2)
    try:
        for slot in (0, 1):
            for bad in fsc.bad_success():
                with pytest.raises(ValueError, match="success must have one entry per read"):
                    pipe.submit(slot, rows, a_s, a_e, success=bad)
            with pytest.raises(ValueError, match="nothing was submitted"):      # the refusals left nothing in flight
                pipe.wait(slot)
            pipe.submit(slot, rows, a_s, a_e, success=ok, want_dist=True, want_fpt=True)
            got = pipe.wait(slot)
            for name in ("status", "call", "dist", "fpt"):
                assert _same(getattr(got, name), getattr(want, name)), (slot, name)
    finally:
        pipe.close()

    # the feeder's parent must not have touched the GPU: a fresh interpreter
    out = str(tmp_path / "feeder.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "feeder_success_check.py"), out],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = np.load(out)
    assert got["refused"].tolist() == [True] * 4 and int(got["free_slots"]) == 4
    good = want_fb.status == 0      # (dwell times and statistics are defined for the reads that succeeded)
    assert _same(got["status"], want_fb.status) and _same(got["fpt"], want_fb.fpt)
    assert _same(got["dwell"][good], want_fb.dwell[good]) and _same(got["stats"][good], want_fb.stats[good])
    assert _same(got["demux_status"], want.status) and _same(got["call"], want.call) and _same(got["dist"], want.dist)
