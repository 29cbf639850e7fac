"""The boundary-detection rule of include/wdx.h ("adapter boundary detection") restated in NumPy, written from the header's text,
and the two trace generators its tests use.  Nothing here calls the library.

  thresholds(p)            thr1, shift_q, var_q as the header converts them (float32 products, clamps)
  detect_one(row, p)       the rule on one float32 row -> dict(a_start, a_end, ok, code, info, gain, g_tie, d_tie)
  detect_rows(rows, p)     ... on every row -> `Expected` (arrays as the entries write them, plus the tie flags)
  synth_trace(seed, i)     open pore | adapter | polyA | body, stride 12 000 with a NaN tail -> (row, true start, true end)
  small_batch(seed, n)     integer-valued pA rows for SMALL parameters, every WDX_DETECT_* code among them
"""
from dataclasses import dataclass

import numpy as np

OK, SHORT, NO_START, NO_ROOM, NO_POLYA = 0, 1, 2, 3, 4
NAN_BITS = 0x7FF8000000000000
_NAN = np.array([NAN_BITS], dtype=np.uint64).view(np.float64)[0]

DEFAULT = dict(max_obs_trace=10000, quant_per_pa=8.0, find_start=1, open_pore_pa=150.0, start_win=32, max_start=2000,
               min_obs_adapter=1000, max_obs_adapter=8000, polya_win=200, step_win=8, refine=300, min_shift_pa=8.0, max_polya_var=9.0)
SMALL = dict(DEFAULT, max_obs_trace=1000, start_win=4, max_start=6, min_obs_adapter=8, max_obs_adapter=40, polya_win=8, step_win=2,
             refine=3)
SMALL_LENGTHS = (0, 1, 19, 20, 21, 63, 64, 65, 127, 129, 1000)
SYNTH_STRIDE = 12000


def thresholds(p):
    f32 = np.float32
    qpp = f32(p["quant_per_pa"])
    with np.errstate(over="ignore"):
        t1 = np.rint(f32(p["open_pore_pa"]) * qpp)
        t2 = np.rint(f32(p["min_shift_pa"]) * qpp)
    thr1 = int(np.minimum(np.maximum(t1, f32(-32768)), f32(32768)))
    shift_q = int(np.minimum(np.maximum(t2, f32(-65536)), f32(65536)))
    v = (np.float64(f32(p["max_polya_var"])) * np.float64(qpp)) * np.float64(qpp)
    var_q = int(min(max(np.floor(v), -1.0), 2147483648.0))
    return thr1, shift_q, var_q


def quantise(x, qpp):
    """q of the leading non-NaN float32 samples x"""
    with np.errstate(over="ignore"):
        v = np.asarray(x, dtype=np.float32) * np.float32(qpp)      # one float32 multiply
    q = np.empty(v.shape, dtype=np.int64)
    hi, lo = v >= np.float32(32767), v <= np.float32(-32768)
    mid = ~(hi | lo)
    q[hi], q[lo] = 32767, -32768
    q[mid] = np.rint(v[mid]).astype(np.int64)                    # round half to even
    return q


def detect_one(row, p):
    row = np.asarray(row, dtype=np.float32)
    sw, pw, tw = int(p["start_win"]), int(p["polya_win"]), int(p["step_win"])
    thr1, shift_q, var_q = thresholds(p)
    cap = min(row.size, int(p["max_obs_trace"]))
    nan = np.flatnonzero(np.isnan(row[:cap]))
    n = int(nan[0]) if nan.size else cap
    out = dict(a_start=-1, a_end=-1, ok=0, code=SHORT, info=[n, -1, -1, -1], gain=_NAN, g_tie=False, d_tie=False)
    if n < sw + int(p["min_obs_adapter"]) + pw:
        return out
    q = quantise(row[:n], p["quant_per_pa"])
    P = np.concatenate(([0], np.cumsum(q)))
    P2 = np.concatenate(([0], np.cumsum(q * q)))
    s = 0
    if p["find_start"]:
        i = np.arange(0, min(int(p["max_start"]), n - sw) + 1)
        hit = (q[i] < thr1) & (P[i + sw] - P[i] < thr1 * sw)
        if not hit.any():
            out["code"] = NO_START
            return out
        s = int(i[np.argmax(hit)])
    out["a_start"] = s
    lo, hi = s + int(p["min_obs_adapter"]), min(n - pw, s + int(p["max_obs_adapter"]))
    if lo > hi:
        out["code"] = NO_ROOM
        return out
    i = np.arange(lo, hi + 1)
    L, R = (P[i] - P[s]).astype(np.float64), (P[n] - P[i]).astype(np.float64)
    g = (L * L) / (i - s).astype(np.float64) + (R * R) / (n - i).astype(np.float64)
    k = int(np.argmax(g))                      # the first maximum
    c = int(i[k])
    out["info"][1], out["gain"], out["g_tie"] = c, g[k], bool((g == g[k]).sum() > 1)
    j = np.arange(max(lo, c - int(p["refine"])), min(hi, c + int(p["refine"])) + 1)
    S1, S2, A1, la = P[j + pw] - P[j], P2[j + pw] - P2[j], P[j] - P[s], j - s
    good = (pw * S2 - S1 * S1 <= var_q * pw * pw) & (S1 * la - A1 * pw >= shift_q * pw * la)
    if not good.any():
        out["code"] = NO_POLYA
        return out
    D = (P[j + tw] - P[j]) - (P[j] - P[j - tw])
    Dg = np.where(good, D, np.iinfo(np.int64).min)
    k = int(np.argmax(Dg))
    e = int(j[k])
    out.update(a_end=e, ok=1, code=OK, d_tie=bool((Dg == Dg[k]).sum() > 1))
    out["info"][2], out["info"][3] = int(P[e] - P[s]), int(P[e + pw] - P[e])
    return out


@dataclass
class Expected:
    a_start: np.ndarray
    a_end: np.ndarray
    ok: np.ndarray
    code: np.ndarray
    info: np.ndarray
    gain: np.ndarray
    g_tie: np.ndarray
    d_tie: np.ndarray

    def take(self, idx):
        return Expected(*[getattr(self, f)[idx] for f in ("a_start", "a_end", "ok", "code", "info", "gain", "g_tie", "d_tie")])


def detect_rows(rows, p, row_len=None):
    """the rule on every row of `rows` (a 2-D array, or a list of 1-D rows); row_len[r] (optional) cuts row r short"""
    res = []
    for r, row in enumerate(rows):
        row = np.asarray(row, dtype=np.float32)
        if row_len is not None:
            row = row[:max(0, min(int(row_len[r]), row.size))]
        res.append(detect_one(row, p))
    n = len(res)
    return Expected(np.array([d["a_start"] for d in res], np.int32).reshape(n), np.array([d["a_end"] for d in res], np.int32).reshape(n),
                    np.array([d["ok"] for d in res], np.uint8).reshape(n), np.array([d["code"] for d in res], np.int32).reshape(n),
                    np.array([d["info"] for d in res], np.int32).reshape(n, 4), np.array([d["gain"] for d in res], np.float64).reshape(n),
                    np.array([d["g_tie"] for d in res], bool).reshape(n), np.array([d["d_tie"] for d in res], bool).reshape(n))


# ---- the synthetic generator ------------------------------------------------------------------------------------------------

def _events(rng, n, level_mean, level_sd, noise_sd):
    """n samples of events of 15..69 samples, levels N(level_mean, level_sd), sample noise N(0, noise_sd)"""
    lens = rng.integers(15, 70, size=n // 15 + 1)
    levels = rng.normal(level_mean, level_sd, size=lens.size)
    return np.repeat(levels, lens)[:n] + rng.normal(0.0, noise_sd, size=n)


def synth_trace(seed, index, stride=SYNTH_STRIDE):
    """Read `index` of the seeded synthetic set -> (float32 row of `stride` samples with a NaN tail, true a_start, true a_end)"""
    rng = np.random.default_rng([int(seed), int(index)])
    n_open, n_ad = int(rng.integers(0, 401)), int(rng.integers(2000, 6001))
    n_pa, n_body = int(rng.integers(400, 3001)), int(rng.integers(300, 2501))
    x = np.concatenate((rng.normal(220.0, 3.0, n_open), _events(rng, n_ad, 80.0, 12.0, 2.5), rng.normal(108.0, 1.2, n_pa),
                        _events(rng, n_body, 95.0, 15.0, 3.0)))[:stride]
    row = np.full(stride, np.nan, dtype=np.float32)
    row[:x.size] = x.astype(np.float32)
    return row, n_open, n_open + n_ad


def synth_batch(seed, n, first=0, stride=SYNTH_STRIDE):
    rows = np.empty((n, stride), dtype=np.float32)
    truth = np.empty((n, 2), dtype=np.int64)
    for i in range(n):
        rows[i], truth[i, 0], truth[i, 1] = synth_trace(seed, first + i, stride)
    return rows, truth


# ---- small parameters: integer-valued pA rows, every code --------------------------------------------------------------------

def small_row(rng, length, kind):
    """`length` integer-valued pA samples (float32) of one of seven kinds"""
    if kind == 0:     # anything in +-4 200 pA (the clamp included)
        x = rng.integers(-4200, 4201, size=length)
    elif kind == 1:   # a constant row: every g ties
        x = np.full(length, int(rng.integers(-200, 140)))
    elif kind == 2:   # open pore throughout
        x = rng.integers(180, 260, size=length)
    elif kind == 6:   # a staircase 98 | 103, 103 | 108: D = 10 pA at three neighbouring j, all of which qualify
        x = np.concatenate((rng.integers(200, 240, int(rng.integers(0, 7))), np.full(int(rng.integers(8, 41)), 98), [103, 103],
                            np.full(int(rng.integers(10, 30)), 108), rng.integers(60, 130, length)))[:length]
    else:             # open pore | adapter | polyA | body, in small steps of noise
        n_open = int(rng.integers(0, 7)) if kind != 5 else int(rng.integers(5, 7))
        n_ad, n_pa = int(rng.integers(8, 41)), int(rng.integers(8, 30))
        amp = 1 if kind == 3 else 3
        x = np.concatenate((rng.integers(200, 240, n_open), 80 + rng.integers(-amp, amp + 1, n_ad),
                            108 + rng.integers(-1, 2, n_pa) * (kind == 4), rng.integers(60, 130, max(0, length))))[:length]
    return x.astype(np.float32)


def small_batch(seed, n, stride=1000):
    """(rows float32 (n, stride) with NaN tails, lengths): the lengths cycle through SMALL_LENGTHS, the kinds are drawn"""
    rng = np.random.default_rng(seed)
    rows = np.full((n, stride), np.nan, dtype=np.float32)
    lengths = np.empty(n, dtype=np.int32)
    for r in range(n):
        length = SMALL_LENGTHS[r % len(SMALL_LENGTHS)] if r % 3 else int(rng.integers(19, 130))
        kind = int(rng.integers(0, 7))
        if r < 4:     # (the batches of 1 and 2 reads hold reads that reach step 4)
            length, kind = (64, 65, 129, 1000)[r], 3
        length = min(length, stride)
        rows[r, :length] = small_row(rng, length, kind)
        lengths[r] = length
    return rows, lengths
