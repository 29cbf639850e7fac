"""Shared pieces of tests/test_gpu_dtw_dispatch.py: the route query, the oracle over several host threads, the
row subsets of the large cases and the inputs with non-finite samples."""
from __future__ import annotations

import contextlib
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import wdx_oracle as orc
from warpdemux_amd import _lib, parallel_distances as pdist

Route = namedtuple("Route", "family band_w exact_w layout fused launches rpb grid_x grid_y window")

RM, TM, RL = "row-major", "read-minor", "refs-as-lanes"


def last_route(ctx=None) -> Route:
    """What the latest DTW dispatch through the context launched (wdx_dtw_last_launch)."""
    i = (ctx or _lib.default_context()).dtw_last_launch()
    return Route(_lib.DTW_FAMILY_NAMES[i.family], i.band_w, bool(i.exact_w), _lib.DTW_LAYOUT_NAMES[i.layout],
                 bool(i.fused_argmin), i.launches, i.refs_per_block, i.grid_x, i.grid_y, i.window)


def kernel_of(r: Route):
    return (r.family, r.band_w, r.exact_w, r.layout)


def effective_window(w, L):
    return L if (w is None or w <= 0 or w > L) else w


def instantiation(w, L, short=True):
    """(family, W, EXACT_W) that serves window w at length L once the wavefront kernel is out of the way: the kernels' own
    domains (wdx_dtw_plan.h: dtw_plan), not a tuning threshold."""
    we = effective_window(w, L)
    if we > 32:
        return ("scratch", 0, False)
    if we == 15:
        return ("short", 15, True) if (L == 25 and short) else ("band", 15, True)
    return ("band", 8 if we <= 8 else 16 if we <= 16 else 32, False)


def fused_rule(nX, nY):
    """dtw_plan folds the argmin into the DTW kernel when one block walks every reference anyway."""
    gx = (nX + 63) // 64
    return gx >= 8 * 3072 or nY == 1 or (gx >= 2048 and nY < 32)


@contextlib.contextmanager
def options(ctx=None, **kw):
    """no_wavefront / no_short / unfused on the context for the duration of the block."""
    ctx = ctx or _lib.default_context()
    opt = {"no_wavefront": _lib.OPT_NO_WAVEFRONT_DTW, "no_short": _lib.OPT_NO_SHORT_DTW, "unfused": _lib.OPT_DTW_UNFUSED}
    for k, v in kw.items():
        ctx.set_option(opt[k], int(v))
    try:
        yield
    finally:
        for k in kw:
            ctx.set_option(opt[k], 0)


ORACLE_THREADS = max(1, min(8, os.cpu_count() or 1))
_pool = None


def oracle_dtw(X, Y, w, p):
    """oracle.wdx_oracle.dtw_matrix, its rows spread over a few host threads (ctypes releases the GIL; the oracle keeps
    no state between calls; its library is loaded here, before any thread asks for it)."""
    global _pool
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0]
    orc.lib()
    with np.errstate(invalid="ignore", over="ignore"):
        if n * Y.shape[0] * X.shape[1] < 200_000:
            return orc.dtw_matrix(X, Y, w, p)
        if _pool is None:
            _pool = ThreadPoolExecutor(max_workers=ORACLE_THREADS)
        parts = np.array_split(np.arange(n), min(n, 4 * ORACLE_THREADS))
        out = list(_pool.map(lambda ix: orc.dtw_matrix(X[ix[0]:ix[-1] + 1], Y, w, p), parts))
    return np.concatenate(out, axis=0)


def subset_rows(n, boundaries=(), seed=0, drawn=2000):
    """Rows of a large case that go to the oracle: the first two waves, the last (partial) wave, the 128 rows around every
    launch / loop boundary and `drawn` rows of a seeded generator."""
    pick = [np.arange(0, min(n, 128)), np.arange(max(0, (n - 1) // 64 * 64), n)]
    for b in boundaries:
        pick.append(np.arange(max(0, b - 64), min(n, b + 64)))
    pick.append(np.random.default_rng(seed).choice(n, min(n, drawn), replace=False))
    return np.unique(np.concatenate(pick))


def read_minor_in_chunks(X, Y, w, p, chunk=4096, want=(TM,)):
    """Second device route of the large cases: the same rows through the transposed (read-minor) form, one launch per
    chunk, separate argmin kernel -- the route the small cases pin to the oracle pair by pair."""
    n = X.shape[0]
    D = np.empty((n, Y.shape[0]), np.float32)
    am = np.empty(n, np.int32)
    with options(no_wavefront=1):
        for r0 in range(0, n, chunk):
            r1 = min(n, r0 + chunk)
            if r1 - r0 < 64:
                r0 = max(0, r1 - 64)      # (a tail of a few rows would go refs-as-lanes: keep a full wave)
            D[r0:r1], am[r0:r1] = pdist.nearest_reference(X[r0:r1], Y, w, p)
            r = last_route()
            assert r.layout in want and r.launches == 1 and r.family != "wavefront", r
    return D, am


def nonfinite_reads(rng, n, L):
    """(n, L) reads, n >= 200: NaN at the first / a middle / the last sample, +inf, -inf, both in one row, inf next to NaN,
    a whole wave of NaN rows (64..127) and a wave with exactly one NaN row (128..191)."""
    assert n >= 200
    X = rng.normal(size=(n, L))
    m = L // 2
    X[1, 0] = np.nan
    X[2, m] = np.nan
    X[3, L - 1] = np.nan
    X[4, m] = np.inf
    X[5, m] = -np.inf
    X[6, 0], X[6, L - 1] = np.inf, -np.inf
    X[7, 0], X[7, L - 1] = np.inf, np.nan
    X[8, :] = np.inf
    X[64:128, m] = np.nan
    X[128 + 17, L - 1] = np.nan
    if n > 4096:
        X[n - 1, 0] = np.nan              # the last lane of the partial wave
        X[rng.choice(np.arange(200, n - 1), 40, replace=False), rng.integers(0, L, 40)] = np.nan
    return X


def nonfinite_refs(rng, L, extra=0):
    """References 0 clean, 1 = copy of 0 (exact tie -> lower index), 2 and 3 clean, 4..6 NaN at the first / middle / last
    sample, then `extra` clean ones.  (A NaN reference column wins every row's argmin, like np.argmin.)"""
    Y = rng.normal(size=(7 + extra, L))
    Y[1] = Y[0]
    Y[4, 0] = np.nan
    Y[5, L // 2] = np.nan
    Y[6, L - 1] = np.nan
    return Y


def equal_infinities(rng, n, L, extra_refs=0):
    """Reads and references that hold the SAME infinity at one index: x[k] - y[k] = inf - inf is NaN inside cell (k, k)
    although no sample is NaN.  dtaidistance's `if (t < minv)` keeps a NaN diagonal predecessor, so the main diagonal stays
    NaN and the distance is NaN; off the diagonal (x[3], y[5]) the NaN cell is never a diagonal predecessor of the last cell
    and the distance is +inf.  Rows 1..6 of both: +inf at k = 0, L // 2, L - 1, then -inf at the same; row 7: +inf at 3
    (reads) / 5 (references); row 8 of the reads: both signs; reference 8 = reference 0 (a finite tie).  The last read
    repeats read 2 (the partial wave of a large batch)."""
    assert n >= 9 and L >= 7
    X, Y = rng.normal(size=(n, L)), rng.normal(size=(9 + extra_refs, L))
    for A in (X, Y):
        for r, (k, v) in enumerate([(0, np.inf), (L // 2, np.inf), (L - 1, np.inf), (0, -np.inf), (L // 2, -np.inf), (L - 1, -np.inf)], 1):
            A[r, k] = v
    X[7, 3], Y[7, 5] = np.inf, np.inf
    X[8, L // 2], X[8, 0] = np.inf, -np.inf
    Y[8] = Y[0]
    if n > 9:
        X[n - 1] = X[2]
    return X, Y
