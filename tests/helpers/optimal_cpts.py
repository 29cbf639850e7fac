"""The optimal change-points of the consensus refinement (WDX_OPT_REFINE_OPTIMAL_CPTS), restated in NumPy, and the
refinement branch composed of the oracle's primitives with either rule for the barcode tail.

`optimal_cpts` is the stated float64 rule of include/wdx.h -- sequential prefix sums, cost(s, t) = (Q[t] - Q[s]) - (P[t] -
P[s])^2 / (t - s), minimum over the pair (value, s) -- what the reference asks ruptures.KernelCPD(kernel="linear",
min_size=m).predict(n_bkps=B) for.  `exact_cost` / `brute_force` evaluate segmentations in exact rational arithmetic.
`refine_one` is sig_proc.py:257-378 + 452-521 read by read: the oracle's clip, t-scores, peak segmentation, event means and
subsequence match, NumPy's statistics, and for the barcode tail either `scores_to_cpts` (the peak branch) or `optimal_cpts`."""
import itertools
from fractions import Fraction

import numpy as np

from oracle import wdx_oracle as orc


def optimal_cpts(x, n_bkps, min_size):
    """[0, b_1 .. b_B, N] or None (infeasible / non-finite sample / min_size < 1)."""
    x = np.asarray(x, dtype=np.float64)
    N, B, m = int(x.size), int(n_bkps), int(min_size)
    if m < 1 or B < 1 or (B + 1) * m > N or not np.isfinite(x).all():
        return None
    P = np.zeros(N + 1)
    Q = np.zeros(N + 1)
    for t in range(N):
        P[t + 1] = P[t] + x[t]
        Q[t + 1] = Q[t] + x[t] * x[t]
    idx = np.arange(N + 1, dtype=np.float64)
    V = np.full(N + 1, np.inf)
    t0 = np.arange(m, N + 1)
    V[t0] = Q[t0] - (P[t0] * P[t0]) / idx[t0]
    path = np.zeros((B + 1, N + 1), dtype=np.int64)
    for k in range(1, B + 1):
        Vn = np.full(N + 1, np.inf)
        for t in range((k + 1) * m, N + 1):
            s = np.arange(k * m, t - m + 1)
            dP = P[t] - P[s]
            c = V[s] + ((Q[t] - Q[s]) - (dP * dP) / (idx[t] - idx[s]))
            j = int(np.argmin(c))   # the first minimum: the smallest s
            Vn[t] = c[j]
            path[k, t] = s[j]
        V = Vn
    b, t = [], N
    for k in range(B, 0, -1):
        t = int(path[k, t])
        b.append(t)
    return np.array([0] + b[::-1] + [N], dtype=np.int64)


def exact_cost(x, cpts):
    """sum over the pieces of sum(v^2) - sum(v)^2 / len, as a Fraction of the float64 samples"""
    tot = Fraction(0)
    for a, b in zip(cpts[:-1], cpts[1:]):
        seg = [Fraction(float(v)) for v in x[int(a):int(b)]]
        tot += sum(v * v for v in seg) - sum(seg) ** 2 / (int(b) - int(a))
    return tot


def brute_force(x, n_bkps, min_size):
    """the exact optimum over every feasible segmentation (None if there is none)"""
    N = len(x)
    best = None
    for bk in itertools.combinations(range(1, N), n_bkps):
        c = [0, *bk, N]
        if min(np.diff(c)) < min_size:
            continue
        e = exact_cost(x, c)
        if best is None or e < best:
            best = e
    return best


def rounding_bound(x):
    """16 N 2^-53 sum(x^2): the accumulated rounding of the two prefix sums"""
    x = np.asarray(x, dtype=np.float64)
    return 16 * x.size * 2.0 ** -53 * float(np.sum(x * x))


def _py_round(v):
    return int(round(v))   # Python's round: half to even, as the reference's int(round(...))


def refine_one(row, a_start, a_end, seg, ref, query, optimal, ok=True, rule="numpy"):
    """One read of the refinement branch -> (status, fpt (K,), dwell (K,), stats (6,), idx (3,)).  seg / ref: the keyword
    dicts of SegParams / RefineParams (sig_extract.normalization "none" only); ``optimal``: the rule of the barcode tail;
    ``rule``: which statement of the optimal rule evaluates it, "numpy" (`optimal_cpts` above) or "c" (the oracle's
    wdx_oracle_optimal_cpts: the same answers, some fifteen times sooner)."""
    cpts_fn = {"numpy": optimal_cpts, "c": orc.optimal_cpts}[rule]
    p = orc.SegParams(**seg)
    r = orc.RefineParams(query=query, **ref)
    assert p.sig_norm == "none"
    K = r.barcode_keep_events
    fpt, dwell, stats, idx = np.full(K, np.nan), np.zeros(K, np.int64), np.full(6, np.nan), np.full(3, -1, np.int32)
    out = lambda st: (st, fpt, dwell, stats, idx)   # noqa: E731
    if not ok:
        return out(1)
    row = np.asarray(row, dtype=np.float32)
    start, stop = max(int(a_start) - p.padding, 0), min(int(a_end) + p.padding, row.size)
    sig = row[start:max(stop, start)].copy()
    n = sig.size
    med, mad = orc.nanmedian_mad_f32(sig)
    if p.clip_bounds_f64:
        tm = float(p.outlier_thresh) * float(mad)
        lo, hi = np.float32(float(med) - tm), np.float32(float(med) + tm)
    else:
        tm = np.float32(p.outlier_thresh) * mad
        lo, hi = np.float32(med - tm), np.float32(med + tm)
    good = ~np.isnan(sig)
    if np.isnan(lo) or np.isnan(hi):
        sig[good] = np.nan
    else:
        v = sig[good]
        v = np.where(v > lo, v, lo)
        v = np.where(v < hi, v, hi)
        sig[good] = v
    E = p.num_events
    d = min(p.min_obs_per_base, _py_round(n / E / 2.0))
    w = min(p.running_stat_width, _py_round(n / E))
    x = sig.astype(np.float64)
    scores = orc.windowed_t_test(x, w)
    try:
        cpts = orc.scores_to_cpts(scores, E, d, w, p.accept_less_cpts)
    except ValueError:
        return out(5)
    if cpts.size == 0 or cpts.size == 1:
        return out(3)
    ev = orc.new_means(x, cpts)
    nseg = ev.size
    if np.isnan(ev).any():
        return out(5)
    with np.errstate(all="ignore"):
        if r.subseq_norm == "mean":
            nrm = (ev - np.mean(ev)) / np.std(ev)
        elif r.subseq_norm == "median":
            m_ = np.median(ev)
            nrm = (ev - m_) / np.median(np.abs(ev - m_))
        else:
            nrm = ev.copy()
    if np.isnan(nrm).any():
        return out(5)
    qs, qe = orc.subseq_match(r.query, nrm, r.penalty, r.psi)
    sbs = int(cpts[qe])
    tail = scores[sbs:]
    if optimal:
        cp2 = cpts_fn(tail, r.barcode_segm_events, p.min_obs_per_base)
        if cp2 is None:
            return out(3)
    else:
        try:
            cp2 = orc.scores_to_cpts(tail, r.barcode_segm_events, p.min_obs_per_base, p.running_stat_width, False)
        except ValueError:
            return out(5)
        if cp2.size == 0:
            return out(3)
        if cp2[-1] != n - sbs:
            return out(5)
    # compute_base_means appends the slice's end when the last boundary is not there: on the optimal branch, which ends at the
    # score curve's end, one more event mean over the last 2 w samples -- B + 2 means beside B + 1 dwell times
    bounds = cp2 if cp2[-1] == n - sbs else np.append(cp2, n - sbs)
    ev2 = orc.new_means(x[sbs:], bounds)
    dw2 = np.diff(cp2)
    nseg2 = dw2.size   # (the engine reports "unknown" where the reference would hand back fewer dwell times than fingerprint entries)
    if p.seg_norm == "mean":
        shift, scale = np.mean(ev), np.std(ev)
    elif p.seg_norm == "median":
        shift = np.median(ev)
        scale = np.median(np.abs(ev - shift))
    else:
        return out(5)
    dt = np.diff(cpts).astype(np.float64)
    dt_med = np.median(dt)
    ev_med = np.median(ev)
    stats[:] = [dt_med, np.median(np.abs(dt - dt_med)), np.mean(ev), np.std(ev), ev_med, np.median(np.abs(ev - ev_med))]
    idx[:] = [qs, qe, sbs]
    assert nseg == cpts.size - 1
    if qs > r.ub_start or qe < r.lb_end or qe > r.ub_end:
        return out(6)
    if nseg2 < K:
        stats[:] = np.nan
        idx[:] = -1
        return out(5)
    with np.errstate(all="ignore"):
        fpt[:] = (ev2[ev2.size - K:] - shift) / scale
    dwell[:] = dw2[nseg2 - K:]
    return out(0)


def refine_batch(sig, a_start, a_end, seg, ref, query, optimal, ok=None, rule="numpy"):
    """`refine_one` over a minibatch -> (fpt, dwell, stats, idx, status), the layout of oracle.fingerprint_refine_batch"""
    res = [refine_one(sig[i], a_start[i], a_end[i], seg, ref, query, optimal, True if ok is None else bool(ok[i]), rule)
           for i in range(len(a_start))]
    return (np.stack([r[1] for r in res]), np.stack([r[2] for r in res]), np.stack([r[3] for r in res]),
            np.stack([r[4] for r in res]), np.array([r[0] for r in res], dtype=np.int32))
