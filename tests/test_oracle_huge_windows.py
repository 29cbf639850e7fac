"""g12: the reference's own detect_results_to_fpt on adapter windows of 16 385 .. 65 536 samples -- beyond
WDX_MAX_ADAPTER_SAMPLES, what ``long_windows=True`` serves (tests/golden/make_golden_huge.py) -- against the CPU oracle, which
has no window limit.  Bit-exact (NaN == NaN): status, fingerprint, dwell times, the six statistics."""
import os

import numpy as np

from oracle import wdx_oracle as orc


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _params_from(g, k):
    pad, sig_norm, d, w, E, acc, seg_norm, K = (int(v) for v in g[f"params_{k}"])
    inv = {0: "none", 1: "mean", 2: "median"}
    return orc.SegParams(padding=pad, sig_norm=inv[sig_norm], outlier_thresh=float(g[f"thresh_{k}"]), min_obs_per_base=d,
                         running_stat_width=w, num_events=E, accept_less_cpts=bool(acc), seg_norm=inv[seg_norm],
                         barcode_num_events=K, clip_bounds_f64=bool(int(g[f"clip64_{k}"])))


def test_g12_huge_adapter_windows_bit_exact(golden_dir):
    g = np.load(os.path.join(golden_dir, "g12_huge_windows.npz"), allow_pickle=False)
    tags, n_ok = set(), 0
    for k in range(int(g["n"])):
        tag = str(g[f"tag_{k}"])
        a_start, a_end, ok = (int(v) for v in g[f"args_{k}"])
        res = orc.fingerprint_one(g[f"row_{k}"], a_start, a_end, _params_from(g, k), ok=bool(ok))
        st_ref = int(g[f"status_{k}"])
        assert res["status"] == st_ref, f"case {k} ({tag}): status {res['status']} != {st_ref}"
        if st_ref == 0:
            n_ok += 1
            assert _same(res["fpt"], g[f"fpt_{k}"]), f"case {k} ({tag}) fpt"
            assert _same(res["dwell"], g[f"dwell_{k}"]), f"case {k} ({tag}) dwell"
            assert _same(res["stats"], g[f"stats_{k}"]), f"case {k} ({tag}) stats"
        tags.add(tag)
    want = {f"{t}_{n}" for t in ("rna004", "rna002", "trna") for n in (16385, 20000, 32768, 65536)}
    want |= {f"rna002_20000_{c}" for c in ("signorm_mean", "segnorm_median", "clip64", "nan_middle", "flat_noise")}
    assert want <= tags and n_ok >= 16


def test_g12_fits_a_committed_file(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "g12_huge_windows.npz")) <= 1 << 20
