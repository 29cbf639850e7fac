"""Inputs of tests/test_gpu_window_edges.py and tests/helpers/feeder_window_check.py: 16 float32 reads in rows of 2 048
samples, adapters at scattered places of their rows (so that a page-locked copy of the batch takes the window pack, not
the 2-D copy), and among them -- the LAST row included -- accepted detections (ok = 1) whose window starts at or beyond
the row's end, an inverted window and a window clipped at both ends.  A short-read parameter set: windows of a few hundred
samples fingerprint to K = 10 events."""
import numpy as np

N, STRIDE, PADDING, K = 16, 2048, 100, 10
SEG = dict(padding=PADDING, min_obs_per_base=4, running_stat_width=8, num_events=30, barcode_num_events=K)
I_AT, I_PLUS1, I_INVERTED, I_CLIPPED, I_PLUS5 = 3, 6, 9, 12, N - 1     # the edge reads; I_PLUS5 is the batch's last row
N_REFS = 4


def batch(seed=7):
    """dict: rows (N, STRIDE) float32 without a NaN tail (every row is full, so nothing hides a read past a row's end),
    a_s / a_e int32, ok uint8 (all 1)."""
    rng = np.random.default_rng(seed)
    rows = np.empty((N, STRIDE), dtype=np.float32)
    a_s, a_e = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    for r in range(N):
        lv = rng.normal(0, 1, 200) * 12.0 + 85.0
        x = np.repeat(lv, rng.integers(8, 20, lv.size))[:STRIDE] + rng.normal(0, 1.5, STRIDE)
        rows[r] = x.astype(np.float32)
        a_s[r] = PADDING + int(rng.integers(0, 1300)) + (r % 4)          # every residue mod 4 of the window start
        a_e[r] = a_s[r] + int(rng.integers(350, 500))
    a_s[I_AT], a_e[I_AT] = STRIDE + PADDING, STRIDE + PADDING + 300               # a_start - padding == stride
    a_s[I_PLUS1], a_e[I_PLUS1] = STRIDE + PADDING + 1, STRIDE + PADDING + 400     # ... == stride + 1
    a_s[I_PLUS5], a_e[I_PLUS5] = STRIDE + PADDING + 5, STRIDE + PADDING + 200     # ... == stride + 5, in the last row
    a_e[I_INVERTED] = a_s[I_INVERTED] - 2 * PADDING - 7                           # a_end < a_start, even with the padding
    a_s[I_CLIPPED], a_e[I_CLIPPED] = 40, STRIDE - 30                              # clipped at both ends: the whole row
    return dict(rows=rows, a_s=a_s, a_e=a_e, ok=np.ones(N, dtype=np.uint8), padding=PADDING)


def windows(b, align=1):
    """(first, stop) of every read by the rule of warpdemux_amd/csrc/wdx_window.h, stated from extract_adapter: the window
    [max(0, a_start - padding), min(stride, a_end + padding)), its start clamped to the row and then rounded down to `align`;
    a dead read or an empty window is (0, 0)"""
    st = np.clip(b["a_s"].astype(np.int64) - b["padding"], 0, STRIDE)
    en = np.minimum(b["a_e"].astype(np.int64) + b["padding"], STRIDE)
    live = (en > st) & b["ok"].astype(bool)
    return np.where(live, st - st % align, 0), np.where(live, en, 0)


def windows_to_box_ratio(b):
    """copied samples over the samples of the column range that holds them all (below 0.85: the window pack)"""
    first, stop = windows(b)
    live = stop > first
    return float((stop - first)[live].sum()) / float((stop[live].max() - first[live].min()) * N)


def pack_rows(b):
    """the rows as a worker packs them: (sig 1-D, row_off, row_len, a_start, a_end) for `wdx_minibatch_in`, rows on 16-byte
    boundaries"""
    first, stop = windows(b, 4)
    pieces, row_off = [], [0]
    for r in range(N):
        piece = np.zeros((stop[r] - first[r] + 3) // 4 * 4, dtype=np.float32)
        piece[: stop[r] - first[r]] = b["rows"][r, first[r]:stop[r]]
        pieces.append(piece)
        row_off.append(row_off[-1] + piece.size)
    return (np.ascontiguousarray(np.concatenate(pieces)), np.array(row_off, dtype=np.int64), (stop - first).astype(np.int32),
            (b["a_s"] - first).astype(np.int32), (b["a_e"] - first).astype(np.int32))


def oracle(b):
    """(fpt, status, refs) of the CPU oracle on the unpacked rows; refs = the first N_REFS successful fingerprints"""
    from oracle import wdx_oracle as orc

    fpt, _dwell, _stats, status = orc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], orc.SegParams(**SEG), b["ok"])
    refs = np.ascontiguousarray(fpt[status == 0][:N_REFS])
    assert refs.shape == (N_REFS, K)
    return fpt, status, refs
