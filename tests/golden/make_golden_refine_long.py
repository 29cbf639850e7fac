"""Fixture g13: detect_results_to_fpt of the REFERENCE with `segmentation.consensus_refinement = True` on adapter windows of
16 385 .. 65 536 samples -- beyond WDX_MAX_ADAPTER_SAMPLES, up to WDX_MAX_LONG_ADAPTER_SAMPLES: what
WDX_OPT_LONG_REFINE_WINDOWS (``fingerprint_refine_batch(..., long_windows=True)``) serves.  The reference has no limit on the
window in either branch (sig_proc.py:382-391, 257-378); a tRNA user gets there with `--export core.max_obs_trace=...`.

Runs only in the build container (needs /root/reference).  The dtaidistance stand-ins and the configuration are
make_golden_refine.py's (imported, not copied: the subsequence match stays parity-unpinned exactly as in g8); the record
layout is g8's, plus `clip64_{k}` (1: the threshold was an np.float64, the clip bounds are evaluated in float64).  The rows
are make_golden_refine.py's `make_read` with the dwell times scaled up to the window length -- random leader | the consensus
shape | 30 barcode events -- rounded to multiples of 1/8 like g12's (a calibrated ADC signal is quantised too): the compressed
file stays below 1 MiB.

    python tests/golden/make_golden_refine_long.py        # writes tests/golden/g13_refine_long.npz
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import make_golden_refine as mgr  # noqa: E402


def long_read(consensus, seed, n, n_lead=8, embed=True, noise=1.5):
    """`make_read` of make_golden_refine.py with its dwell times (14 .. 59 samples) scaled so that the read has exactly `n`
    samples (the rounding's remainder goes to the first leader level), on the 1/8 grid"""
    r = np.random.Generator(np.random.PCG64(seed))
    lv = list(r.normal(0, 1, n_lead))
    lv += list(consensus if embed else r.normal(0, 1, consensus.size))
    lv += list(r.normal(0, 1, 30))
    lv = np.array(lv) * 12.0 + 85.0
    dw = r.integers(14, 60, lv.size)
    dw = np.maximum(dw * n // int(dw.sum()), 1)
    dw[0] += n - int(dw.sum())
    assert dw[0] > 0 and int(dw.sum()) == n
    x = np.repeat(lv, dw) + r.normal(0, noise, n)
    return (np.round(x * 8.0) / 8.0).astype(np.float32)


def main():
    sp, DetectResults, _, _ = mg.import_reference()
    sp.warping_paths_fast = mgr.warping_paths_fast
    sp.SubsequenceAlignment = mgr.SubsequenceAlignment
    consensus = np.load(os.path.join(HERE, "g8_refine.npz"))["consensus"]   # (the reference's 84-point consensus, as g8 recorded it)
    g = {"consensus": consensus}
    k = 0

    def run_case(row, a_start, a_end, tag, **kw):
        nonlocal k
        spc = mgr.make_spc(**kw)
        dr = DetectResults(success=True, fail_reason="", adapter_start=a_start, adapter_end=a_end)
        work = np.array(row, dtype=np.float32, copy=True)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = sp.detect_results_to_fpt(work, spc, dr, consensus)
            st = mg.status_code(res) if res.fail_reason != "consensus query outlier" else 6
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
        norm = {"none": 0, "mean": 1, "median": 2}
        g[f"row_{k}"] = np.array(row, dtype=np.float32)
        g[f"args_{k}"] = np.array([a_start, a_end], dtype=np.int64)
        g[f"seg_{k}"] = np.array([spc.sig_extract.padding, s.min_obs_per_base, s.running_stat_width, s.num_events,
                                  norm[s.normalization], s.barcode_num_events[0], s.barcode_num_events[1],
                                  norm[s.consensus_subseq_match_normalization],
                                  *[int(v) for v in s.consensus_subseq_match_psi], s.consensus_subseq_match_ub_start,
                                  s.consensus_subseq_match_lb_end, s.consensus_subseq_match_ub_end], dtype=np.int64)
        g[f"fl_{k}"] = np.array([spc.core.sig_norm_outlier_thresh, s.consensus_subseq_match_penalty], dtype=np.float64)
        g[f"clip64_{k}"] = np.int64(isinstance(spc.core.sig_norm_outlier_thresh, np.float64))
        g[f"status_{k}"] = np.int64(st)
        g[f"fpt_{k}"], g[f"dwell_{k}"], g[f"stats_{k}"], g[f"idx_{k}"] = fpt, dwell, stats, idx
        g[f"tag_{k}"] = np.array(tag)
        print(k, tag, "status", st, "idx", idx)
        k += 1
        return st

    sts = []
    # the window is the whole row: a_start = padding, a_end = n - padding
    for i, n in enumerate((16385, 20000, 32769, 49152, 65536)):
        sts.append(run_case(long_read(consensus, 100 + i, n), 100, n - 100, f"embedded_{n}"))
    sts.append(run_case(long_read(consensus, 200, 20000, embed=False), 100, 19900, "no_consensus_20000"))
    sts.append(run_case(long_read(consensus, 201, 32769), 100, 32669, "clip64_32769", thresh=np.float64(2.7)))
    sts.append(run_case(long_read(consensus, 202, 20000), 100, 19900, "median_norms_20000", seg_norm="median", sub_norm="median"))
    g["n"] = np.int64(k)
    dst = os.path.join(HERE, "g13_refine_long.npz")
    np.savez_compressed(dst, **g)
    print(dst, os.path.getsize(dst), "bytes; status histogram:", {s: sts.count(s) for s in sorted(set(sts))})
    assert os.path.getsize(dst) <= 1 << 20, "a committed file is at most 1 MiB: drop the 49 152-sample length first"
    assert sts.count(0) >= 5, "the long windows with the consensus embedded are meant to refine"


if __name__ == "__main__":
    main()
