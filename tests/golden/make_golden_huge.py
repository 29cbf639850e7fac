"""Fixture g12: detect_results_to_fpt of the REFERENCE on adapter windows of 16 385 .. 65 536 samples -- beyond
WDX_MAX_ADAPTER_SAMPLES, up to WDX_MAX_LONG_ADAPTER_SAMPLES: what WDX_OPT_LONG_WINDOWS (``long_windows=True``) serves --
for the three shipped parameter triples (num_events, min_obs_per_base, running_stat_width): RNA004 (110, 6, 12),
RNA002 (110, 15, 30), tRNA (120, 9, 18).  The reference has no limit on the window (sig_proc.py:382-391); a user gets
there with `--export core.max_obs_trace=...`.

Runs only in the build container (needs /root/reference); same recipe and record layout as make_golden_long.py's g4b.
The rows are make_golden_long.long_row's, rounded to multiples of 1/8 (a calibrated ADC signal is quantised too): the
compressed file stays below 1 MiB with every length in it.

    python tests/golden/make_golden_huge.py        # writes tests/golden/g12_huge_windows.npz
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden_long import long_row  # noqa: E402

LENGTHS = (16385, 20000, 32768, 49152, 65536)


def huge_row(rng, n, mean_dwell):
    return (np.round(long_row(rng, n, mean_dwell).astype(np.float64) * 8.0) / 8.0).astype(np.float32)


def main():
    sp, DetectResults, _, _ = mg.import_reference()
    rng = np.random.Generator(np.random.PCG64(20261018))
    g, k = {}, 0

    def run_case(row, a_start, a_end, tag, **spc_kw):
        nonlocal k
        spc = mg.make_spc(**spc_kw)
        dr = DetectResults(success=True, fail_reason="", adapter_start=a_start, adapter_end=a_end)
        row_in = np.array(row, dtype=np.float32, copy=True)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = sp.detect_results_to_fpt(row_in.copy(), spc, dr)
            st = mg.status_code(res)
        except Exception:  # barcode_fpt_wrapper -> "unknown"
            res, st = None, 5
        K = spc.segmentation.barcode_num_events
        fpt, dwell, stats = np.full(K, np.nan), np.zeros(K, dtype=np.int64), np.full(6, np.nan)
        if st == 0:
            fpt[:] = res.barcode_fpt
            dwell[:] = res.dwell_times
            stats[:] = [res.adapter_dt_med, res.adapter_dt_mad, res.adapter_event_mean, res.adapter_event_std,
                        res.adapter_event_med, res.adapter_event_mad]
        p = spc
        g[f"row_{k}"] = row_in
        g[f"args_{k}"] = np.array([a_start, a_end, 1], dtype=np.int64)
        g[f"params_{k}"] = np.array(
            [p.sig_extract.padding, {"none": 0, "mean": 1, "median": 2}[p.sig_extract.normalization],
             p.segmentation.min_obs_per_base, p.segmentation.running_stat_width, p.segmentation.num_events,
             int(p.segmentation.accept_less_cpts), {"none": 0, "mean": 1, "median": 2}[p.segmentation.normalization],
             K], dtype=np.int64)
        g[f"thresh_{k}"] = np.float64(p.core.sig_norm_outlier_thresh)
        g[f"clip64_{k}"] = np.int64(isinstance(p.core.sig_norm_outlier_thresh, np.float64))
        g[f"status_{k}"] = np.int64(st)
        g[f"fpt_{k}"], g[f"dwell_{k}"], g[f"stats_{k}"] = fpt, dwell, stats
        g[f"tag_{k}"] = np.array(tag)
        print(k, tag, "status", st)
        k += 1

    triples = {"rna004": dict(E=110, d=6, w=12), "rna002": dict(E=110, d=15, w=30), "trna": dict(E=120, d=9, w=18)}
    # the window is the whole row: a_start = padding, a_end = n - padding
    for n in LENGTHS:
        row = huge_row(rng, n, n / 135.0)
        for name, t in triples.items():
            run_case(row, 100, n - 100, f"{name}_{n}", **t)
    row = huge_row(rng, 20000, 20000 / 135.0)
    run_case(row, 100, 19900, "rna002_20000_signorm_mean", sig_norm="mean", **triples["rna002"])
    run_case(row, 100, 19900, "rna002_20000_segnorm_median", seg_norm="median", **triples["rna002"])
    run_case(row, 100, 19900, "rna002_20000_clip64", thresh=np.float64(2.7), **triples["rna002"])
    nm = row.copy()
    nm[9000:9004] = np.nan
    run_case(nm, 100, 19900, "rna002_20000_nan_middle", **triples["rna002"])
    run_case((np.round((80 + rng.normal(0, 1, 20000)) * 8.0) / 8.0).astype(np.float32), 100, 19900, "rna002_20000_flat_noise",
             **triples["rna002"])
    g["n"] = np.int64(k)
    dst = os.path.join(HERE, "g12_huge_windows.npz")
    np.savez_compressed(dst, **g)
    print(dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) <= 1 << 20, "a committed file is at most 1 MiB: drop the 49 152-sample length first"


if __name__ == "__main__":
    main()
