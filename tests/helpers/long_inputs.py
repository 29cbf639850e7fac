"""Inputs of the long-window tests (tests/test_gpu_long_windows.py, tests/helpers/feeder_long_check.py): adapter windows
around WDX_MAX_ADAPTER_SAMPLES = 16 384 and up to (and beyond) WDX_MAX_LONG_ADAPTER_SAMPLES = 65 536 samples, which
``long_windows=True`` (WDX_OPT_LONG_WINDOWS) serves."""
import os

import numpy as np

from helpers import adc_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
PADDING = 100
CAP, LONG_CAP = 16384, 65536
TRIPLES = {"rna004": dict(num_events=110, min_obs_per_base=6, running_stat_width=12),
           "rna002": dict(num_events=110, min_obs_per_base=15, running_stat_width=30),
           "trna": dict(num_events=120, min_obs_per_base=9, running_stat_width=18)}
K = 25


def step_row(rng, n, mean_dwell=None):
    """a step signal with geometric-ish dwell times (>= 8 samples), white noise and a few flicker spikes -- about 135 levels
    per window unless ``mean_dwell`` says otherwise -- on a grid of 1/8 (tests/golden/make_golden_huge.py's rows)"""
    mean_dwell = n / 135.0 if mean_dwell is None else mean_dwell
    dw = 8 + rng.geometric(1.0 / max(mean_dwell - 8.0, 1.5), size=int(2 * n / mean_dwell) + 64)
    lv = 80.0 + 15.0 * rng.normal(size=dw.size)
    s = np.repeat(lv, dw)[:n]
    assert s.size == n
    s = s + rng.normal(0, 2.0, n)
    idx = rng.integers(0, n, max(1, n // 1000))
    s[idx] += rng.choice([-60.0, 60.0], idx.size)
    return (np.round(s * 8.0) / 8.0).astype(np.float32)


def quiet_row(rng, n, steps):
    """`steps` noise-free levels of random lengths: the score curve is zero between the steps, so a window has about `steps`
    peaks -- fewer than num_events: "event segmentation failed" unless accept_less_cpts"""
    cuts = np.sort(rng.choice(np.arange(200, n - 200, 40), steps - 1, replace=False))
    lv = np.round((80.0 + 15.0 * rng.normal(size=steps)) * 8.0) / 8.0
    return np.repeat(lv, np.diff(np.concatenate([[0], cuts, [n]]))).astype(np.float32)


def minibatch(rows):
    stride = max(r.size for r in rows)
    mb = np.full((len(rows), stride), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        mb[i, : r.size] = r
    return mb


# the window lengths of the edge batch: both sides of the exact kernel's LDS capacity (11 200), of the default cap, of a
# multiple of 64 behind it, of 32 768 (the peak list's chunks go from 32 to 33 positions per thread) and of the long cap
EDGE_LENGTHS = (3000, 11201, 16384, 16385, 16386, 16447, 16448, 20000, 32767, 32768, 32769, 65535, 65536, 65537, 70000)


def edge_batch():
    """dict rows (n, stride) float32 with NaN tails, a_s, a_e, ok, win (the window each read's bounds select): the 15 lengths
    above as whole-row windows, then a window that runs into its row's NaN tail, a failed detection, adapters that start
    inside the padding (short and long), a NaN run inside a long window, flat noise, long dwells, bounds at the row's ends, and
    two windows with fewer change-points than events"""
    rng = np.random.default_rng(20261018)
    rows, a_s, a_e, ok = [], [], [], []

    def add(row, s, e, good=1):
        rows.append(row)
        a_s.append(s)
        a_e.append(e)
        ok.append(good)

    for n in EDGE_LENGTHS:
        add(step_row(rng, n), PADDING, n - PADDING)
    add(step_row(rng, 20000), PADDING, 20000 + 57)               # 15: a_end + padding beyond the samples: NaN tail
    add(step_row(rng, 30000), PADDING, 30000 - PADDING, 0)       # 16: ok = 0
    add(step_row(rng, 5000), 30, 5000 - PADDING)                 # 17: a_start < padding (short)
    add(step_row(rng, 40000), 30, 40000 - PADDING)               # 18: a_start < padding (long)
    r = step_row(rng, 24000)
    r[12000:12004] = np.nan
    add(r, PADDING, 24000 - PADDING)                             # 19: NaN run in the middle of a long window
    add((np.round((80 + rng.normal(0, 1, 33000)) * 8.0) / 8.0).astype(np.float32), PADDING, 33000 - PADDING)   # 20: flat noise
    add(step_row(rng, 50000, 50000 / 60.0), PADDING, 50000 - PADDING)    # 21: fewer levels than events
    add(step_row(rng, 18000, 18000 / 60.0), PADDING, 18000 - PADDING)    # 22: the same, shorter
    add(step_row(rng, 16500), 0, 16500)                          # 23: bounds at the row's ends: window 16 600 with 100 NaN
    add(quiet_row(rng, 9000, 60), 0, 9000 - PADDING)             # 24: fewer change-points than events (accept_less_cpts), short
    add(quiet_row(rng, 26000, 70), PADDING, 26000 - PADDING)     # 25: ... and long
    mb = minibatch(rows)
    a_s, a_e = np.array(a_s, dtype=np.int32), np.array(a_e, dtype=np.int32)
    win = np.minimum(a_e + PADDING, mb.shape[1]) - np.maximum(a_s - PADDING, 0)
    return dict(rows=mb, a_s=a_s, a_e=a_e, ok=np.array(ok, dtype=np.uint8), win=win)


def g12():
    return np.load(os.path.join(GOLDEN, "g12_huge_windows.npz"), allow_pickle=False)


def ways_batch():
    """The 12 reads every way in is shown, RNA002 triple: seven rows of fixture g12 (16 385 .. 65 536 samples, flat
    noise among them) and five of 3 000 .. 40 001 samples, quantised to int16 (tests/helpers/adc_inputs.py) so that the float32 rows
    ARE `sig_proc.calibrate_adc` of the int16 rows.  -> dict adc / row_len / offset / scale / rows / a_s / a_e / ok"""
    g = g12()
    tags = {str(g[f"tag_{k}"]): k for k in range(int(g["n"]))}
    rows = [g[f"row_{tags[t]}"] for t in ("rna002_16385", "rna002_20000", "rna002_32768", "rna002_49152", "rna002_65536",
                                          "rna002_20000_clip64", "rna002_20000_flat_noise")]
    rng = np.random.default_rng(12)
    rows += [step_row(rng, n) for n in (3000, 11201, 16384, 17000, 40001)]
    mb = minibatch(rows)
    assert mb.shape == (12, LONG_CAP)
    adc, row_len, offset, scale = adc_inputs.quantise(mb, 13)
    from warpdemux_amd import sig_proc

    cal = sig_proc.calibrate_adc(adc, row_len, offset, scale)
    a_s = np.full(12, PADDING, dtype=np.int32)
    a_e = (row_len - PADDING).astype(np.int32)
    a_s[7] = 30                                 # the padding is cropped
    a_e[10] = row_len[10] + 20                  # into the NaN tail: a window of 17 120 samples, 120 of them NaN
    ok = np.ones(12, dtype=np.uint8)
    ok[8] = 0
    return dict(adc=adc, row_len=row_len, offset=offset, scale=scale, rows=cal, a_s=a_s, a_e=a_e, ok=ok)


WAYS_SEG = dict(padding=PADDING, barcode_num_events=K, **TRIPLES["rna002"])
