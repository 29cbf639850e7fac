"""Run by tests/test_gpu_boost_paths.py in a FRESH interpreter (the parent of a Feeder must not have touched the GPU): a
ring laid out for 3 classes served by a context whose resident DTW_SVM has 4 -- the smallest one tests/helpers/svm_ref.py
builds, one support vector per class.  A minibatch of 2 reads with WDX_WANT_SVM through wdx_feeder_run and 2 fingerprints
through wdx_feeder_predict must both be answered WDX_ERR_INVALID with the two class counts in the message, nothing of the
4-class model written into the 3-class slot; the same minibatch without the tail bit is then served (fingerprints against
the oracle bit for bit, the call against the oracle's distances), and every slot is free at the end.  Prints one JSON
line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from helpers import svm_ref  # noqa: E402
from oracle import wdx_oracle as orc  # noqa: E402
from warpdemux_amd import sig_proc, synth  # noqa: E402
from warpdemux_amd.feeder import Feeder  # noqa: E402

K = 25
N_SLOTS = 2


def refused(call):
    try:
        call()
        return "served"
    except ValueError as e:
        return str(e)
    except Exception as e:  # noqa: BLE001
        return type(e).__name__ + ": " + str(e)


if __name__ == "__main__":
    spec = synth.SynthSpec(n_barcodes=4)
    mb, a_s, a_e, _ = synth.generate_minibatch(spec, 0, 6, 8000)
    fpt, dwell, stats, status = orc.fingerprint_batch(mb, a_s, a_e, orc.SegParams(barcode_num_events=K))
    assert (status == 0).all()
    X_train = np.ascontiguousarray(fpt[2:])     # four references; the minibatch is the two reads in front of them
    rows, r_s, r_e = mb[:2], a_s[:2], a_e[:2]
    model = svm_ref.synth_model(4, seed=3, n_support=[1, 1, 1, 1], n_extra=0).to_dtw_svm(X_train)
    # Feeder derives the ring's n_classes from its model, so the geometry is patched for the time this feeder is created
    import warpdemux_amd.feeder as fmod

    fmod._lib.load()     # (binds the library's prototypes to the real record first)
    real_geo = fmod._lib.FeederGeometryC

    def geo_with_three_classes(n_slots, n_events, n_classes, *rest):
        return real_geo(n_slots, n_events, 3, *rest)

    fmod._lib.FeederGeometryC = geo_with_three_classes
    try:
        with Feeder(model=model, params=sig_proc.SegParams(barcode_num_events=K), max_reads=2, stride=8000,
                    n_slots=N_SLOTS) as odd:
            odd.n_classes = 3      # the worker's outputs are sized like the ring
            rec = {"model_classes": int(model.n_classes),
                   "run": refused(lambda: odd.detect_and_predict(rows, r_s, r_e)),
                   "predict": refused(lambda: odd.predict(fpt[:2])),
                   "run_again": refused(lambda: odd.detect_and_predict(rows, r_s, r_e))}
            fb = odd.fingerprint_batch(rows, r_s, r_e)
            db = odd.demux_batch(rows, r_s, r_e)
            D = orc.dtw_matrix(fpt[:2], X_train, 15, 0.1)
            rec["served_without_the_tail"] = bool(
                np.array_equal(fb.status, status[:2]) and np.array_equal(fb.fpt.view(np.uint64), fpt[:2].view(np.uint64))
                and np.array_equal(fb.dwell, dwell[:2]) and np.array_equal(fb.stats.view(np.uint64), stats[:2].view(np.uint64))
                and np.array_equal(db.status, status[:2]) and np.array_equal(db.call, np.argmin(D, axis=1))
                and np.allclose(db.dist, D, rtol=1e-5, atol=0))
            rec["alive"] = bool(odd.alive())
            rec["stats"] = odd.stats()
    finally:
        fmod._lib.FeederGeometryC = real_geo
    print(json.dumps(rec))
