"""The edge table of the one-wave-per-tile DTW kernels (medoid_tile_kernel, self_tile_kernel, loo_tile_kernel), what each row of it
stands for, and the inputs of tests/test_gpu_tile_edges.py and tests/test_tile_edges_host.py.

The two classifiers below are written from the headers' statements (wdx_medoid_plan.h: medoid_kernel; wdx_dtw_tile.h:
medoid_band_cost), in plain Python: nothing of the library is imported.

INPUTS.  Self matrix and leave-one-out share `loo_input(L)`: helpers.loo_rule.rows(L, 200) -- four chunks of 64 rows, so 4 diagonal
and 6 strictly upper tiles -- and the medoids take `medoid_input(L)`: helpers.medoid_rule.labelled_rows(L), whose labels of 65, 129
and 200 rows have strictly upper tiles.  Both go through `with_small_rows`, which scales some member rows far down (see there);
every special row of the two generators keeps its role.

WHAT THE INPUTS HOLD AT L = 1 AND L = 2.  The generators normalise each centre to zero mean, so at L = 1 every centre is 0 and a
row is one noise sample; nothing else changes: the "NaN at L // 3" sample is sample 0, the "inf at L - 1" sample is sample 0 at
L = 1 and sample 1 at L = 2, and the two sit in DIFFERENT rows (14 and 90; for the medoids the 11th row of label 4 and the 78th of
label 5), so no role coincides with another.  Row 100 x 1e160 still overflows float32 against every row, the copies of row 10 still
tie at +0.0, and the rows scaled by 1e-41 still lie in the float32 denormal range (one sample of about 1e-41 each)."""
import functools

import numpy as np

from helpers import loo_rule, medoid_rule

# ---- the table ---------------------------------------------------------------------------------------------------------------------
# name: (L, window, penalty); window None is an unbanded call (effective window L)
EDGES = {
    # window 15, the exact kernel: the masked path (L < 28) ...
    "w15_L15": (15, 15, 0.1),
    "w15_L16": (16, 15, 0.1),
    "w15_L26": (26, 15, 0.1),
    "w15_L27": (27, 15, 0.1),
    "w15_L25_short": (25, 15, 0.1),       # the unrolled short kernel
    "w15_L25_no_short": (25, 15, 0.1),    # the same shape under WDX_OPT_NO_SHORT_DTW: the masked path of the band-15 kernel
    # ... and the schedule in pieces: head | chunks of 8 with a prefetch | remainder | tail
    "w15_L28": (28, 15, 0.1),
    "w15_L29": (29, 15, 0.1),
    "w15_L35": (35, 15, 0.1),
    "w15_L36": (36, 15, 0.1),
    "w15_L37": (37, 15, 0.1),
    "w15_L43": (43, 15, 0.1),             # (one chunk and the longest remainder)
    "w15_L44": (44, 15, 0.1),
    "w15_L45": (45, 15, 0.1),
    "w15_L52": (52, 15, 0.1),             # (three chunks, no remainder: `more` true twice, xn never reloaded)
    "w15_L110_p0": (110, 15, 0.0),
    # band16: effective windows 9 .. 14 and 16
    "b16_40_9": (40, 9, 0.1),
    "b16_40_12": (40, 12, 0.1),
    "b16_40_14": (40, 14, 0.1),
    "b16_40_16": (40, 16, 0.1),
    "b16_110_16": (110, 16, 0.1),
    "b16_33_16_p0": (33, 16, 0.0),
    "b16_12_over": (12, 15, 0.1),         # the window is larger than L: w = 12
    "b16_16_unbanded": (16, None, 0.1),
    # band8: effective windows 1 .. 8
    "b8_40_1": (40, 1, 0.1),
    "b8_40_8": (40, 8, 0.1),
    "b8_5_over": (5, 15, 0.1),            # w = 5
    "b8_1_unbanded": (1, None, 0.1),
    "b8_2_unbanded": (2, None, 0.1),
    "b8_8_unbanded": (8, None, 0.1),
    "b8_40_3_p0": (40, 3, 0.0),
    # band32: effective windows 17 .. 32
    "b32_110_17": (110, 17, 0.1),
    "b32_110_24": (110, 24, 0.1),
    "b32_110_31": (110, 31, 0.1),
    "b32_40_20": (40, 20, 0.1),
    "b32_17_unbanded": (17, None, 0.1),
    "b32_32_unbanded": (32, None, 0.1),
    "b32_70_32_p0": (70, 32, 0.0),
    # the route edge: the general route by the window rule alone, no option set
    "gen_33_unbanded": (33, None, 0.1),
    "gen_110_33": (110, 33, 0.1),
}
NO_SHORT = frozenset(["w15_L25_no_short"])             # rows that run under WDX_OPT_NO_SHORT_DTW
FAMILIES = ("medoids", "self_matrix", "loo")
MODES = (0, 1, 2)                                       # WDX_OPT_DTW_UNFUSED
BAND16_SMALL_N = (1, 2, 63, 64, 65, 129)                # the chunk edges, band16 rows, self matrix and leave-one-out
ROUTE_ROWS = ("b16_40_12", "w15_L28", "w15_L36", "w15_L44", "b32_32_unbanded")   # tile route against the forced general route
GENERAL_ROWS = ("gen_33_unbanded", "gen_110_33")

MAX_REG_WINDOW = 32


def effective_window(L, window):
    return L if (window is None or window <= 0 or window > L) else window


def kernel_of(L, window, no_short=False):
    """the MedoidKernel that serves (L, window) with no *_GENERAL option set: short | band8 | band15 | band16 | band32 | general"""
    w = effective_window(L, window)
    if w > MAX_REG_WINDOW:
        return "general"
    if L == 25 and w == 15 and not no_short:
        return "short"
    if w == 15:
        return "band15"
    return "band8" if w <= 8 else ("band16" if w <= 16 else "band32")


def schedule_of(L, W=15):
    """the row schedule of the exact window-W kernel at length L: ("masked", head_rows, body_rows, tail_rows) when L < 2 (W - 1),
    else ("pieces", whole_chunks, remainder_rows, prefetches) of the L - 2 (W - 1) body rows between W - 1 head and W - 1 tail rows"""
    if L < 2 * (W - 1):
        head_end = min(W - 1, L)
        body_end = max(head_end, L - W + 1)
        return ("masked", head_end, body_end - head_end, L - body_end)
    body = L - 2 * (W - 1)
    chunks = body // 8
    return ("pieces", chunks, body % 8, max(chunks - 1, 0))


def row_kernel(name):
    L, window, _ = EDGES[name]
    return kernel_of(L, window, name in NO_SHORT)


def cases():
    """every (family, row, mode) of tests/test_gpu_tile_edges.py"""
    return [(f, r, m) for f in FAMILIES for r in EDGES for m in MODES]


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
# the rows of helpers.loo_rule.rows that have a role of their own
SPECIAL_ROWS = (10, 14, 20, 50, 60, 80, 90, 100, 110, 120, 140, 160, 180, 194, 195)
SCALE_DENORMAL = 1e-41   # distances between two such rows are about 1e-40: float32 denormals
SCALE_ZERO = 1e-170      # every squared difference of two such rows underflows float64: the distance is exactly +0.0
SCALE_TINY = 1e-150      # squared differences of about 1e-300: a nonzero sum below 1e-280 (the settle rule runs the pair again), +0.0f


def small_rows(X, labels, status=None, avoid=SPECIAL_ROWS):
    """(denormal, zero, tiny): the rows `with_small_rows` scales.  A and B are the two labels with the most eligible rows (a member
    that `avoid` does not name; the lower label among equals): for the medoids' input the labels of 200 and 129 rows.  With q the
    eligible rows of a label in rising order:
        denormal  A: the first, the middle and the last of q;  B: the first and the last        (five rows, two labels)
        zero      A: q at one and at three quarters;  B: the middle                            (three rows, two labels)
        tiny      A: the two rows of q right behind the three-quarter row                       (two rows, behind every zero row of A)
    so that in row order (the chunks of the self matrix and of leave-one-out) and in order within the label (the chunks of the
    medoids) each set spans more than one chunk wherever the label does."""
    X, labels = np.asarray(X), np.asarray(labels)
    ok = np.isfinite(X).all(axis=1) & (labels >= 0)
    if status is not None:
        ok &= np.asarray(status) == 0
    ok[[r for r in avoid if r < len(ok)]] = False
    labs, counts = np.unique(labels[ok], return_counts=True)
    order = np.lexsort((labs, -counts))
    if len(order) < 2 or counts[order[1]] < 3 or counts[order[0]] < 9:
        raise ValueError("with_small_rows needs two labels of at least 9 and 3 eligible rows, not %r" % dict(zip(labs.tolist(), counts.tolist())))
    qa, qb = (np.flatnonzero(ok & (labels == labs[k])) for k in order[:2])
    ma, three = len(qa) // 2, (3 * len(qa)) // 4
    denormal = [qa[0], qa[ma], qa[-1], qb[0], qb[-1]]
    zero = [qa[len(qa) // 4], qa[three], qb[len(qb) // 2]]
    tiny = [qa[three + 1], qa[three + 2]]
    picked = denormal + zero + tiny
    if len(set(int(r) for r in picked)) != len(picked):
        raise ValueError("with_small_rows: the labels are too small for ten distinct rows")
    return tuple(np.array(sorted(int(r) for r in s), dtype=np.int64) for s in (denormal, zero, tiny))


def with_small_rows(X, labels, status=None, avoid=SPECIAL_ROWS):
    """a copy of X in which the rows of `small_rows` are scaled by 1e-41 (five rows), 1e-170 (three) and 1e-150 (two)"""
    denormal, zero, tiny = small_rows(X, labels, status, avoid)
    X = np.array(X, dtype=np.float64, copy=True)
    X[denormal] *= SCALE_DENORMAL
    X[zero] *= SCALE_ZERO
    X[tiny] *= SCALE_TINY
    return X


def zero_neighbours(labels, zero):
    """(row, side, neighbour) for every 1e-170 row and side that holds another 1e-170 row: the lowest such row"""
    out = []
    for a in zero:
        for side in (0, 1):
            cand = [b for b in zero if b != a and (labels[b] == labels[a]) == (side == 0)]
            if cand:
                out.append((int(a), side, int(min(cand))))
    return out


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def loo_input(L, n=loo_rule.N_ROWS):
    """(X, labels, status) of the self matrix and of leave-one-out; the small rows are in the 200-row form only (the forms of
    n < 130 rows hold no special row at all)"""
    X, labels, status = loo_rule.rows(L, n)
    if n == loo_rule.N_ROWS:
        X = with_small_rows(X, labels, status)
    return _frozen(X, labels, status)


@functools.lru_cache(maxsize=None)
def medoid_input(L):
    """(X, labels, status, n_labels) of the medoids"""
    X, labels, status, G = medoid_rule.labelled_rows(L)
    X = with_small_rows(X, labels, status, avoid=())
    return _frozen(X, labels, status) + (G,)
