"""Inputs of the int16 ADC tests (tests/test_gpu_adc.py, tests/helpers/feeder_adc_check.py): synthetic minibatches
quantised to int16 the way a pod5 file holds them -- per-read ``scale`` near 0.1755 and per-read ``offset`` that differ
between reads, ``row_len`` from the generator's rows -- plus the cases the int16 way in has to get right: windows that run
past the read's end into the NaN tail, failed detections, inverted windows, adapter starts at every residue mod 8, and
windows at the fingerprint kernels' capacity edges."""
import numpy as np

from warpdemux_amd import synth

PADDING = 100


def quantise(mb, seed):
    """(adc int16 (n, stride), row_len, offset, scale): the int16 samples whose calibration is closest to ``mb``."""
    n = mb.shape[0]
    rng = np.random.default_rng(seed)
    scale = (0.1755 * (1.0 + 0.02 * rng.uniform(-1, 1, n))).astype(np.float32)
    offset = (-240.0 + rng.uniform(-20, 20, n)).astype(np.float32)      # non-integer, different for every read
    row_len = np.isfinite(mb).sum(axis=1).astype(np.int32)               # the generator's rows: samples, then the NaN tail
    assert all(np.isfinite(mb[i, :row_len[i]]).all() for i in range(n))
    q = np.rint(np.nan_to_num(mb.astype(np.float64)) / scale[:, None].astype(np.float64) - offset[:, None].astype(np.float64))
    adc = np.clip(q, -32768, 32767).astype(np.int16)
    adc[np.arange(mb.shape[1])[None, :] >= row_len[:, None]] = 12345      # whatever the file's buffer held: never read
    return adc, row_len, offset, scale


def main_batch(n=256, stride=9000, first=770_000):
    """Whole reads with jittered adapter starts; returns a dict of the minibatch's arrays."""
    spec = synth.SynthSpec(n_barcodes=10)
    mb, a_s, a_e, _ = synth.generate_minibatch(spec, first, n, stride, start_jitter=700)
    adc, row_len, offset, scale = quantise(mb, 5)
    a_s, a_e = a_s.copy(), a_e.copy()
    ok = np.ones(n, dtype=np.uint8)
    ok[5::23] = 0                                  # failed detections ...
    a_s[28] = 2_000_000                            # ... one of them with a garbage start far outside the row
    ok[28] = 0
    a_e[3::19] += 57                               # a_end + padding beyond row_len: the window runs into the NaN tail
    a_e[11] = a_s[11] - 5                          # inverted window
    a_e[12] = a_s[12] - 2 * PADDING - 1            # ... inverted even with the padding
    a_s[40] = stride + 500                         # an accepted detection whose window starts beyond the row
    a_e[40] = stride + 900
    assert len(set(((a_s - PADDING) % 8).tolist())) == 8, "adapter starts at every residue mod 8"
    assert (a_e[3::19].astype(np.int64) + PADDING > row_len[3::19]).all()
    b = dict(adc=adc, row_len=row_len, offset=offset, scale=scale, a_s=a_s, a_e=a_e, ok=ok, padding=PADDING)
    assert windows_to_box_ratio(b) < 0.8, "a page-locked copy of this minibatch must take the window pack over the bus"
    return b


def long_batch():
    """Windows at the capacity edges of the fingerprint kernels (5 120 / 6 144 / 8 192 / 16 384), one of 16 385 samples
    (status 5) and a few beside the edges; padding 0, the window is the whole read."""
    rng = np.random.default_rng(12)
    lens = [5120, 6144, 8192, 16384, 16385, 5119, 6145, 8193, 11200, 4000]
    n, stride = len(lens), 16392
    mb = np.full((n, stride), np.nan, dtype=np.float32)
    for i, ln in enumerate(lens):
        mb[i, :ln] = (np.repeat(rng.normal(80, 15, ln // 40 + 1), 40)[:ln] + rng.normal(0, 2, ln)).astype(np.float32)
    adc, row_len, offset, scale = quantise(mb, 6)
    assert row_len.tolist() == lens
    b = dict(adc=adc, row_len=row_len, offset=offset, scale=scale, a_s=np.zeros(n, dtype=np.int32),
             a_e=np.array(lens, dtype=np.int32), ok=None, padding=0)
    assert windows_to_box_ratio(b) < 0.8, "a page-locked copy of this minibatch must take the window pack over the bus"
    return b


def windows_to_box_ratio(b):
    """samples inside the adapter windows over samples of the column range that holds them all: below 0.85 a page-locked
    minibatch is read window by window over the bus (pack_windows_adc_kernel), from there on by the 2-D copy"""
    n, stride = b["adc"].shape
    st = np.clip(b["a_s"].astype(np.int64) - b["padding"], 0, stride) & ~7
    en = np.minimum(np.minimum(b["a_e"].astype(np.int64) + b["padding"], stride), b["row_len"])
    live = (en > st) & (np.ones(n, bool) if b["ok"] is None else b["ok"].astype(bool))
    return float((en - st)[live].sum()) / float((en[live].max() - st[live].min()) * n)


def pack_rows(b):
    """The rows of a minibatch packed the way a feeder worker packs them (int16 windows only, rows on 16-byte boundaries):
    (adc 1-D, row_off, row_len, row_win, a_start, a_end) for `sig_proc.adc_minibatch` / `MinibatchPipeline.submit_adc`."""
    adc, pad = b["adc"], b["padding"]
    n, stride = adc.shape
    pieces, row_off, r_len, r_win, a_s2, a_e2 = [], [0], [], [], [], []
    for r in range(n):
        s0 = min(max(int(b["a_s"][r]) - pad, 0), stride)
        e0 = min(int(b["a_e"][r]) + pad, stride)
        dead = b["ok"] is not None and not b["ok"][r]
        if e0 <= s0 or dead:
            s0 = win = valid = 0
        else:
            s0 &= ~7
            win = e0 - s0
            valid = min(max(int(b["row_len"][r]) - s0, 0), win)
        piece = np.zeros((valid + 7) // 8 * 8, dtype=np.int16)
        piece[:valid] = adc[r, s0:s0 + valid]
        pieces.append(piece)
        row_off.append(row_off[-1] + piece.size)
        r_len.append(valid)
        r_win.append(win)
        a_s2.append(int(b["a_s"][r]) - s0)
        a_e2.append(int(b["a_e"][r]) - s0)
    flat = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.int16)
    return (np.ascontiguousarray(flat), np.array(row_off, dtype=np.int64), np.array(r_len, dtype=np.int32),
            np.array(r_win, dtype=np.int32), np.array(a_s2, dtype=np.int32), np.array(a_e2, dtype=np.int32))
