"""Inputs of the refine-path tests (tests/test_gpu_refine_paths.py, tests/helpers/feeder_refine_check.py): the tRNA
parameter set and the consensus query of fixture g8 (as tests/test_gpu_refine.py uses them) on seeded synthetic reads of
2 500 .. 6 000 samples whose adapters start at different samples of their rows, quantised to int16 the way
tests/helpers/adc_inputs.py does it, so that the float32 rows ARE `sig_proc.calibrate_adc` of the int16 rows.

Every batch holds, by construction, the reads the host paths have to get right: a failed detection (ok = 0), a window far
too short (status 3), reads without the consensus (status 6), a window that runs past the read's end into the NaN tail, an
adapter that starts at sample 0 (the padding is cropped) -- and, in the float32 rows only (int16 has no NaN), a NaN inside
a window."""
import os

import numpy as np

from helpers import adc_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
PADDING = 100
SEG = dict(padding=PADDING, min_obs_per_base=9, running_stat_width=18, num_events=120)
REF = dict(barcode_segm_events=25, barcode_keep_events=25)
I_DEAD, I_NAN, I_SHORT, I_TAIL, I_ZERO, I_CROP = 5, 7, 9, 11, 13, 14   # the special reads of every batch


def consensus():
    return np.load(os.path.join(GOLDEN, "g8_refine.npz"))["consensus"]


def batch(seed, n=96):
    """dict: adc / row_len / offset / scale (int16 form), rows (their calibration: float32, NaN tail), rows_nan (rows with
    a NaN inside read I_NAN's window), a_s / a_e / ok, padding."""
    q = consensus()
    rng = np.random.default_rng(seed)
    reads, lead = [], []
    for i in range(n):
        emb = i % 6 != 4                                   # every sixth read carries no consensus: an outlier
        lv = np.concatenate([rng.normal(0, 1, int(rng.integers(2, 34))), q if emb else rng.normal(0, 1, q.size),
                             rng.normal(0, 1, 30)]) * 12.0 + 85.0
        dw = rng.integers(12, 40, lv.size)
        x = np.repeat(lv, dw) + rng.normal(0, rng.uniform(0.8, 3.0), int(dw.sum()))
        junk = 0 if i in (I_ZERO, I_CROP) else int(rng.integers(0, 1200))       # the adapter starts anywhere in its row
        reads.append(np.concatenate([rng.normal(85, 12, junk), x]).astype(np.float32))
        lead.append(junk)
    sizes = np.array([r.size for r in reads])
    assert sizes.min() >= 2500 and sizes.max() <= 6000, (sizes.min(), sizes.max())
    stride = int(sizes.max()) + 200
    mb = np.full((n, stride), np.nan, dtype=np.float32)
    for i, r in enumerate(reads):
        mb[i, : r.size] = r
    adc, row_len, offset, scale = adc_inputs.quantise(mb, seed + 1)
    a_s = np.array(lead, dtype=np.int32) + PADDING
    a_e = (sizes - PADDING).astype(np.int32)
    ok = np.ones(n, dtype=np.uint8)
    ok[I_DEAD] = 0
    a_e[I_SHORT] = a_s[I_SHORT] + 900                      # far too short: too few peaks
    a_e[I_TAIL] += 157                                     # a_end + padding beyond the read: into the NaN tail
    a_s[I_ZERO] = 0                                        # window start -100 -> 0: the padding is cropped
    a_s[I_CROP] = 37
    from warpdemux_amd import sig_proc

    rows = sig_proc.calibrate_adc(adc, row_len, offset, scale)
    rows_nan = rows.copy()
    rows_nan[I_NAN, a_s[I_NAN] + 1500: a_s[I_NAN] + 1504] = np.nan
    assert int(a_e[I_TAIL]) + PADDING > row_len[I_TAIL] and int(a_e[I_TAIL]) + PADDING <= stride
    b = dict(adc=adc, row_len=row_len, offset=offset, scale=scale, rows=rows, rows_nan=rows_nan, a_s=a_s, a_e=a_e, ok=ok,
             padding=PADDING)
    assert adc_inputs.windows_to_box_ratio(b) < 0.8, "a page-locked copy of this minibatch must take the window pack"
    return b


def check_kinds(status, with_nan):
    """every kind of read the batch was built to hold did occur"""
    st = np.asarray(status)
    assert st[I_DEAD] == 1 and st[I_SHORT] == 3 and st[I_TAIL] != 0, st[[I_DEAD, I_SHORT, I_TAIL]]
    assert st[I_ZERO] in (0, 6) and st[I_CROP] in (0, 6), st[[I_ZERO, I_CROP]]
    assert (st == 6).sum() >= 3 and (st == 0).sum() >= 40, np.bincount(st, minlength=8)
    if with_nan:
        assert st[I_NAN] not in (0, 6), st[I_NAN]


def pack_rows_f32(b, rows):
    """The float32 rows packed the way a feeder worker packs them: row r = samples [st & ~3, en) of the caller's row, rows
    on 16-byte boundaries -> (sig 1-D, row_off, row_len, a_start, a_end) for `wdx_minibatch_in`."""
    n, stride = rows.shape
    pieces, row_off, r_len, a_s2, a_e2 = [], [0], [], [], []
    for r in range(n):
        s0 = max(int(b["a_s"][r]) - b["padding"], 0)
        e0 = min(int(b["a_e"][r]) + b["padding"], stride)
        if e0 < s0 or not b["ok"][r]:
            e0 = s0
        s0 &= ~3
        piece = np.zeros((e0 - s0 + 3) // 4 * 4, dtype=np.float32)
        piece[: e0 - s0] = rows[r, s0:e0]
        pieces.append(piece)
        row_off.append(row_off[-1] + piece.size)
        r_len.append(e0 - s0)
        a_s2.append(int(b["a_s"][r]) - s0)
        a_e2.append(int(b["a_e"][r]) - s0)
    return (np.ascontiguousarray(np.concatenate(pieces)), np.array(row_off, dtype=np.int64), np.array(r_len, dtype=np.int32),
            np.array(a_s2, dtype=np.int32), np.array(a_e2, dtype=np.int32))
