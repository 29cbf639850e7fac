"""Golden vectors of the consensus-refinement branch with ``segmentation.refinement_optimal_cpts = True``
(sig_proc.py:348-354; WDX_OPT_REFINE_OPTIMAL_CPTS).

Runs only in the build container.  As for g8 (make_golden_refine.py) the reference's own `detect_results_to_fpt` is executed:
its adapter segmentation, the slicing of the score tail, `np.insert(valid_cpts, 0, 0)`, `compute_base_means`, `normalize_wrt`,
stats and outlier filter are the REFERENCE's code.  Two library calls it cannot make here are stand-ins: the dtaidistance pair
of make_golden_refine.py, and `ruptures.KernelCPD`, replaced by a NumPy class of the stated float64 rule
(tests/helpers/optimal_cpts.py; include/wdx.h) -- so the fixture pins everything AROUND the call, and the optimum itself
stays PARITY UNPINNED against the real library.

One stated deviation: where ruptures raises (BadSegmentationParameters: the tail cannot hold B + 1 pieces of min_size) the
reference's call dies; the engine reports "event segmentation failed" (status 3), and so does this fixture.

    python tests/golden/make_golden_optimal.py      # writes tests/golden/g14_refine_optimal.npz
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, ROOT, import_reference, status_code  # noqa: E402
from make_golden_refine import SubsequenceAlignment, make_spc, warping_paths_fast  # noqa: E402


class BadSegmentationParameters(Exception):
    pass


class KernelCPD:
    """ruptures.KernelCPD(kernel="linear", min_size=m): fit(signal (N, 1)), predict(n_bkps) -> [b_1 .. b_B, N]"""

    def __init__(self, kernel="linear", min_size=2, **kw):
        assert kernel == "linear" and not kw
        self.min_size = int(min_size)

    def fit(self, signal):
        self.x = np.asarray(signal, dtype=np.float64).reshape(-1)
        return self

    def predict(self, n_bkps=None, pen=None):
        from helpers.optimal_cpts import optimal_cpts

        assert pen is None
        cp = optimal_cpts(self.x, int(n_bkps), self.min_size)
        if cp is None:
            raise BadSegmentationParameters
        return [int(v) for v in cp[1:]]


def main():
    sys.path.insert(0, ROOT)
    sp, DetectResults, _, _ = import_reference()
    sp.warping_paths_fast = warping_paths_fast
    sp.SubsequenceAlignment = SubsequenceAlignment
    sp.KernelCPD = KernelCPD
    consensus = np.load(os.path.join(HERE, "g8_refine.npz"))["consensus"]

    rng = np.random.Generator(np.random.PCG64(20251014))
    g = {"consensus": consensus}
    k = 0

    def make_read(seed, n_lead=8, embed=True, noise=1.5, dwell_lo=14, dwell_hi=60):
        r = np.random.Generator(np.random.PCG64(seed))
        lv = list(r.normal(0, 1, n_lead))
        lv += list(consensus if embed else r.normal(0, 1, consensus.size))
        lv += list(r.normal(0, 1, 30))
        lv = np.array(lv) * 12.0 + 85.0
        dw = r.integers(dwell_lo, dwell_hi, lv.size)
        x = np.repeat(lv, dw) + r.normal(0, noise, int(dw.sum()))
        return x.astype(np.float32)

    def run_case(row, a_start, a_end, tag, **kw):
        nonlocal k
        spc = make_spc(**kw)
        spc.segmentation.refinement_optimal_cpts = True
        dr = DetectResults(success=True, fail_reason="", adapter_start=a_start, adapter_end=a_end)
        work = np.array(row, dtype=np.float32, copy=True)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = sp.detect_results_to_fpt(work, spc, dr, consensus)
            st = status_code(res) if res.fail_reason != "consensus query outlier" else 6
        except BadSegmentationParameters:
            res, st = None, 3   # the stated deviation
        except Exception:
            res, st = None, 5
        K = spc.segmentation.barcode_num_events[1]
        fpt, dwell, stats, idx = np.full(K, np.nan), np.zeros(K, np.int64), np.full(6, np.nan), np.full(3, -1, np.int64)
        if st in (0, 6):
            stats[:] = [res.adapter_dt_med, res.adapter_dt_mad, res.adapter_event_mean, res.adapter_event_std,
                        res.adapter_event_med, res.adapter_event_mad]
            idx[:] = [res.seg_cons_query_start, res.seg_cons_query_end, res.sig_barcode_start]
        if st == 0:
            fpt[:] = res.barcode_fpt
            dwell[:] = res.dwell_times
        s = spc.segmentation
        codes = {"none": 0, "mean": 1, "median": 2}
        g[f"row_{k}"] = np.array(row, dtype=np.float32)
        g[f"args_{k}"] = np.array([a_start, a_end], dtype=np.int64)
        g[f"seg_{k}"] = np.array([spc.sig_extract.padding, s.min_obs_per_base, s.running_stat_width, s.num_events,
                                  codes[s.normalization], s.barcode_num_events[0], s.barcode_num_events[1],
                                  codes[s.consensus_subseq_match_normalization], *[int(v) for v in s.consensus_subseq_match_psi],
                                  s.consensus_subseq_match_ub_start, s.consensus_subseq_match_lb_end,
                                  s.consensus_subseq_match_ub_end], dtype=np.int64)
        g[f"fl_{k}"] = np.array([spc.core.sig_norm_outlier_thresh, s.consensus_subseq_match_penalty], dtype=np.float64)
        g[f"status_{k}"] = np.int64(st)
        g[f"fpt_{k}"], g[f"dwell_{k}"], g[f"stats_{k}"], g[f"idx_{k}"] = fpt, dwell, stats, idx
        g[f"tag_{k}"] = np.array(tag)
        k += 1
        return st

    sts = []
    for i in range(5):
        x = make_read(1100 + i, n_lead=int(rng.integers(2, 16)))
        sts.append(run_case(x, 100, x.size - 100, "embedded"))
    for i in range(2):   # consensus far into the read: outliers of the filter
        x = make_read(2100 + i, n_lead=int(rng.integers(25, 40)))
        sts.append(run_case(x, 100, x.size - 100, "late_consensus"))
    x = make_read(4100)
    sts.append(run_case(x, 100, x.size - 100, "median_norms", seg_norm="median", sub_norm="median"))
    x = make_read(5100)
    sts.append(run_case(x, 100, x.size - 100, "wide_filter_keep20", ub_start=60, lb_end=0, ub_end=200, bne=(25, 20)))
    x = make_read(5200)
    sts.append(run_case(x, 100, x.size - 100, "min_size_3_twelve_bkps", ub_start=60, lb_end=0, ub_end=200, d=3, bne=(12, 13)))
    # (the two reads below keep the parameters of the first seven, so that nine reads make one minibatch)
    # short adapter: the window width shrinks below the configured one -- this branch never leaves the slice
    x = make_read(7101, n_lead=4, dwell_lo=8, dwell_hi=16)
    sts.append(run_case(x, 100, x.size - 100, "shrunk_width"))
    # a tail that cannot hold 26 pieces of 9 samples
    x = make_read(8100)
    cut = x.size - 31 * 30
    sts.append(run_case(x[:cut], 100, cut - 100, "infeasible_tail"))
    g["n"] = np.int64(k)
    np.savez_compressed(os.path.join(HERE, "g14_refine_optimal.npz"), **g)
    print("G14 cases:", k, "status histogram:", {s: sts.count(s) for s in sorted(set(sts))}, sts)


if __name__ == "__main__":
    main()
