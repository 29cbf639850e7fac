"""Fixture g11: detect_results_to_fpt of the REFERENCE over the segmentation parameter domain the engine accepts
beyond the shipped triples -- num_events 1 .. 253, barcode_num_events up to 254, running_stat_width 0 .. 64,
min_obs_per_base 0 .. 1000 (suppression reach beyond 17), "mean" / "median" / "none" segment normalisation, "median"
signal normalisation, short windows whose parameters shrink (sig_proc.py:526-533) with n/E and n/2E on .5 ties,
and windows of 11 200 / 11 201 / 16 384 samples.

Rows are float step signals from seeded NumPy (no quantisation: exact score ties would make the reference's
np.argsort order decide).  Runs only where the reference checkout make_golden.import_reference loads is present; same
recipe and record layout as make_golden.py's G4.

    python tests/golden/make_golden_domain.py        # writes tests/golden/g11_param_domain.npz
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402


def step_row(rng, n, mean_dwell):
    """step signal with geometric dwell times (>= 3 samples) and white noise"""
    lo = min(3.0, mean_dwell - 1.0)
    k = int(n / max(lo, 1.0)) + 2
    dw = lo + rng.geometric(1.0 / max(mean_dwell - lo, 1.0), k)
    lv = 80.0 + 15.0 * rng.normal(size=k)
    s = np.repeat(lv, dw.astype(np.int64))[:n]
    return (s + rng.normal(0, 2.0, n)).astype(np.float32)


def main():
    sp, DetectResults, _, _ = mg.import_reference()
    rng = np.random.Generator(np.random.PCG64(20261016))
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
        print(k, tag, "n", a_end - a_start, "status", st)
        k += 1

    def case(tag, n, E, d, w, K, dwell=None, pad=0, **kw):
        """one read: an n-sample adapter window (+ pad samples of row on either side, taken as padding)"""
        dw = dwell if dwell is not None else max(4.0, 0.75 * n / max(E, 1))
        row = step_row(rng, n + 2 * pad, dw)
        run_case(row, pad, n + pad, tag, padding=pad, E=E, d=d, w=w, K=K, **kw)

    # fast-gate edges: kFSeg = 128 segments, e_magic1 saturation (E = 1, 2), reach 17 / 18, width 36 / 37
    case("E126_K127", 3000, 126, 6, 12, 127)
    case("E127_K25", 3000, 127, 6, 12, 25)
    case("E1_K2", 900, 1, 6, 12, 2, dwell=40.0)
    case("E2_K3", 900, 2, 6, 12, 3, dwell=40.0)
    for d in (17, 18):
        case(f"d{d}_w30", 4400, 110, d, 30, 25, pad=100)
    for w in (36, 37):
        case(f"d6_w{w}", 3000, 110, 6, w, 25)
    case("d18_w12", 4400, 110, 18, 12, 25)
    # exact-kernel interior: up to 254 segments, reach up to 40, widths up to 64
    case("E200_K201", 5000, 200, 6, 12, 201)
    for norm in ("mean", "median", "none"):
        case(f"E253_K254_segnorm_{norm}", 6000, 253, 6, 12, 254, seg_norm=norm)
    case("E253_d3_w6", 4000, 253, 3, 6, 25)
    case("d25_w30", 5000, 110, 25, 30, 25)
    case("d30_w30_K110", 7000, 110, 30, 30, 110, dwell=40.0)
    case("E200_d20_w40_K200", 9000, 200, 20, 40, 200, dwell=30.0)
    case("E60_d40_w48", 5000, 60, 40, 48, 25, dwell=50.0)
    for w in (63, 64):
        case(f"d9_w{w}", 3000, 110, 9, w, 25)
    case("E253_d40_w64_K254_accept_less", 8000, 253, 40, 64, 254, accept_less=True)
    # long suppression reach at width 12 (the shrink caps it at round(n / 2E) = 75); the first 2 900 samples are flat
    # (less than half: the MAD stays > 0; a wide clip threshold), so the rest holds fewer than E peaks that far apart:
    # "event segmentation failed" unless accept_less_cpts
    for d in (64, 200, 1000):
        row = step_row(rng, 6000, 60.0)
        row[:2900] = np.float32(80.0)
        for acc in (False, True):
            run_case(row, 0, 6000, f"E40_d{d}_accept_less{int(acc)}", padding=0, E=40, d=d, w=12, K=10,
                     thresh=50.0, accept_less=acc)
    for w in (1, 2, 3, 4, 5):
        case(f"d3_w{w}", 2000, 110, 3, w, 25)
    # settings the reference fails on
    case("d0", 2000, 110, 0, 12, 25)
    case("w0", 2000, 110, 6, 0, 25)
    case("K_E_plus_2", 2000, 60, 6, 12, 62)
    # signal normalisation
    case("E200_K201_signorm_median", 5000, 200, 6, 12, 201, pad=100, sig_norm="median")
    # short windows: the parameter shrink binds; n/E or n/2E exactly on .5 (round half to even)
    for n, E, d in ((1155, 110, 17), (1265, 110, 17), (1925, 110, 17), (2090, 110, 6), (2310, 110, 17),
                    (2277, 253, 17), (3795, 253, 6), (1000, 200, 17), (3400, 200, 17), (945, 126, 17),
                    (420, 20, 17), (460, 20, 17), (430, 20, 6), (870, 20, 17), (630, 30, 17), (690, 30, 6)):
        case(f"short_{n}_E{E}_d{d}", n, E, d, 36, min(E + 1, 25), dwell=4.0)
    # windows at the exact kernel's LDS capacity and the engine's limit (fingerprint_big_kernel beyond 11 200)
    case("E200_d20_w40_K200_11200", 11200, 200, 20, 40, 200)
    case("E200_d20_w40_K200_11201", 11201, 200, 20, 40, 200)
    case("E253_K254_11201", 11201, 253, 6, 12, 254)
    case("E253_d25_w30_K254_16384", 16384, 253, 25, 30, 254, dwell=20.0, accept_less=True)
    g["n"] = np.int64(k)
    dst = os.path.join(HERE, "g11_param_domain.npz")
    np.savez_compressed(dst, **g)
    sts = [int(g[f"status_{i}"]) for i in range(k)]
    print(dst, os.path.getsize(dst), "bytes;", k, "cases; status histogram:", {s: sts.count(s) for s in sorted(set(sts))})


if __name__ == "__main__":
    main()
