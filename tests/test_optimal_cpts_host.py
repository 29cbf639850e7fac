"""Optimal change-points of the consensus refinement (WDX_OPT_REFINE_OPTIMAL_CPTS), the parts that need no GPU: the NumPy
restatement of the rule (tests/helpers/optimal_cpts.py) against brute force in exact arithmetic, its ties, the oracle's C
statement of the same rule (wdx_oracle_optimal_cpts, the fast reference of tests/test_gpu_optimal_batch.py) against the NumPy
one with no tolerance, the refinement branch composed of the oracle's primitives against the oracle (peak rule) and against
fixture g14 (optimal rule, through either statement), and the constructor rules of the Python layer."""
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

from helpers import optimal_cpts as oc
from oracle import wdx_oracle as orc
from test_oracle_refine import params_from
from warpdemux_amd import _lib, sig_proc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_restatement_against_brute_force_in_exact_arithmetic():
    """200 random cases, N <= 12: feasibility agrees, and the exact cost of the float64 answer is within the accumulated
    rounding of the two prefix sums, 16 N 2^-53 sum(x^2), of the exact optimum over every feasible segmentation."""
    rng = np.random.default_rng(20251014)
    worst, n_feasible = 0.0, 0
    for _ in range(200):
        N, m, B = int(rng.integers(4, 13)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        x = rng.normal(size=N) * 3
        cp = oc.optimal_cpts(x, B, m)
        assert (cp is not None) == ((B + 1) * m <= N)
        if cp is None:
            assert oc.brute_force(x, B, m) is None
            continue
        n_feasible += 1
        assert cp[0] == 0 and cp[-1] == N and cp.size == B + 2 and np.diff(cp).min() >= m
        gap = float(oc.exact_cost(x, cp) - oc.brute_force(x, B, m))
        assert 0 <= gap <= oc.rounding_bound(x), (gap, oc.rounding_bound(x))
        worst = max(worst, gap / oc.rounding_bound(x))
    assert n_feasible >= 100
    print("worst gap / bound:", worst)


def test_ties_go_to_the_smallest_start():
    assert oc.optimal_cpts(np.zeros(40), 3, 9).tolist() == [0, 9, 18, 27, 40]
    assert oc.optimal_cpts(np.repeat([1.0, 5.0, 2.0, 7.0], 10), 3, 9).tolist() == [0, 10, 20, 30, 40]


def test_failures_of_the_rule():
    x = np.arange(20.0)
    assert oc.optimal_cpts(x, 1, 11) is None and oc.optimal_cpts(x, 1, 10).tolist() == [0, 10, 20]
    assert oc.optimal_cpts(x, 1, 0) is None
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7] = bad
        assert oc.optimal_cpts(y, 2, 3) is None


def _both(x, B, m):
    """the two statements of the rule on one series: identical arrays or both None; -> the answer"""
    a, c = oc.optimal_cpts(x, B, m), orc.optimal_cpts(x, B, m)
    assert (a is None) == (c is None), (len(x), B, m, a, c)
    if a is not None:
        assert c.dtype == np.int64 and c.shape == (B + 2,) and a.tolist() == c.tolist(), (len(x), B, m, a.tolist(), c.tolist())
    return c


def _series(rng, N, grid):
    """noisy steps; ``grid``: levels and noise on the integers, so that costs tie exactly"""
    n_steps = int(rng.integers(1, 12))
    lv = np.repeat(rng.normal(0, 4, n_steps), -(-N // n_steps))[:N]
    if grid:
        return np.round(lv) + rng.integers(-1, 2, N).astype(np.float64)
    return lv + rng.normal(0, 1, N)


def test_c_statement_equals_the_numpy_statement_on_seeded_series():
    """330 series, N in 4 .. 600 (small N favoured: the NumPy statement costs B N Python steps), B in 1 .. 40, m in 1 .. 12,
    every third series on an integer grid; about one in eight infeasible.  No tolerance: the same arrays."""
    rng = np.random.default_rng(20260114)
    n_ok = n_none = 0
    seen_N, seen_B, seen_m = set(), set(), set()
    for i in range(330):
        N = (4, 600)[i] if i < 2 else int(4 + 596 * rng.random() ** 3)
        m = (1, 12)[i] if i < 2 else int(rng.integers(1, min(12, max(1, N // 3)) + 1))
        fit = N // m - 1                                  # the largest feasible B
        if i < 2:
            B = (1, 40)[i]
        elif i % 8 == 5 or fit < 1:
            B = int(min(40, max(1, fit + int(rng.integers(1, 4)))))
        else:
            B = int(rng.integers(1, min(40, fit) + 1))
        got = _both(_series(rng, N, i % 3 == 0), B, m)
        assert (got is not None) == ((B + 1) * m <= N)
        if got is None:
            n_none += 1
        else:
            n_ok += 1
            assert got[0] == 0 and got[-1] == N and np.diff(got).min() >= m
        seen_N.add(N), seen_B.add(B), seen_m.add(m)
    assert n_ok >= 250 and n_none >= 20, (n_ok, n_none)
    assert {4, 600} <= seen_N and {1, 40} <= seen_B and seen_m == set(range(1, 13))


def test_c_statement_at_the_cap_of_the_change_points_and_at_every_feasibility_edge():
    rng = np.random.default_rng(7)
    for N, m in ((253, 1), (254, 1), (255, 1), (600, 1), (600, 2), (507, 2), (508, 2)):      # B = 253, barcode_segm_events' cap
        assert (_both(_series(rng, N, N % 2 == 0), 253, m) is not None) == (254 * m <= N)
    for B, m in ((1, 1), (1, 12), (3, 9), (7, 5), (25, 9), (40, 1), (40, 12)):
        for N in ((B + 1) * m - 1, (B + 1) * m, (B + 1) * m + 1):
            for grid in (False, True):
                got = _both(_series(rng, N, grid), B, m)
                assert (got is not None) == (N >= (B + 1) * m)
                if N == (B + 1) * m:
                    assert got.tolist() == list(range(0, N + 1, m)), "one feasible segmentation"


def test_c_statement_ties_constants_and_failures():
    assert _both(np.zeros(40), 3, 9).tolist() == [0, 9, 18, 27, 40]
    assert _both(np.repeat([1.0, 5.0, 2.0, 7.0], 10), 3, 9).tolist() == [0, 10, 20, 30, 40]
    for x in (np.full(77, 2.5), np.full(300, -1e6), np.zeros(210), np.full(5, 1e-300)):
        for B, m in ((1, 1), (4, 1), (5, 5), (3, 2)):
            _both(x, B, m)
    x = np.arange(20.0)
    assert orc.optimal_cpts(x, 1, 11) is None and orc.optimal_cpts(x, 1, 10).tolist() == [0, 10, 20]
    assert orc.optimal_cpts(x, 1, 0) is None and orc.optimal_cpts(x, 1, -3) is None
    assert orc.optimal_cpts(x, 0, 3) is None and orc.optimal_cpts(x, -1, 3) is None
    assert orc.optimal_cpts(np.zeros(0), 1, 1) is None and orc.optimal_cpts(np.zeros(1), 1, 1) is None
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 7, 19):
            y = x.copy()
            y[at] = bad
            assert _both(y, 2, 3) is None


def _reads(consensus, n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        emb = rng.random() > 0.2
        lv = np.concatenate([rng.normal(0, 1, int(rng.integers(2, 34))), consensus if emb else rng.normal(0, 1, consensus.size),
                             rng.normal(0, 1, 30)]) * 12.0 + 85.0
        dw = rng.integers(12, 40, lv.size)
        rows.append((np.repeat(lv, dw) + rng.normal(0, rng.uniform(0.8, 3.0), int(dw.sum()))).astype(np.float32))
    stride = max(r.size for r in rows)
    mb = np.full((n, stride), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        mb[i, : r.size] = r
    return mb, np.full(n, 100, dtype=np.int32), np.array([r.size - 100 for r in rows], dtype=np.int32)


def test_composition_with_the_peak_rule_is_the_oracle(golden_dir):
    """option off: the helper's composition (oracle primitives + scores_to_cpts) == oracle.fingerprint_refine_batch, on the
    reads of fixture g8 (its shrunk width, too few peaks and short tail included) and on a seeded minibatch"""
    g = np.load(os.path.join(golden_dir, "g8_refine.npz"))
    seen = set()
    for k in range(int(g["n"])):
        seg, ref = params_from(g, k)
        row = g[f"row_{k}"]
        a_s, a_e = (int(v) for v in g[f"args_{k}"])
        st, fpt, dwell, stats, idx = oc.refine_one(row, a_s, a_e, seg, ref, g["consensus"], optimal=False)
        o = orc.fingerprint_refine_batch(row.reshape(1, -1), [a_s], [a_e], orc.SegParams(**seg),
                                         orc.RefineParams(query=g["consensus"], **ref))
        assert st == int(o[4][0]) == int(g[f"status_{k}"]), (k, st, o[4][0])
        seen.add(st)
        assert _same(fpt, o[0][0]) and _same(dwell, o[1][0]), k
        if st in (0, 6):
            assert _same(stats, o[2][0]) and _same(idx, o[3][0]), k
    assert {0, 3, 5, 6} <= seen
    mb, a_s, a_e = _reads(g["consensus"], 24, 3)
    mb[7, 2000:2004] = np.nan
    ok = np.ones(24, np.uint8)
    ok[5] = 0
    seg = dict(min_obs_per_base=9, running_stat_width=18, num_events=120, barcode_num_events=25)
    ref = dict(barcode_segm_events=25, barcode_keep_events=25)
    h = oc.refine_batch(mb, a_s, a_e, seg, ref, g["consensus"], optimal=False, ok=ok)
    o = orc.fingerprint_refine_batch(mb, a_s, a_e, orc.SegParams(**seg), orc.RefineParams(query=g["consensus"], **ref), ok=ok)
    assert _same(h[4], o[4]) and _same(h[0], o[0]) and _same(h[1], o[1])
    rep = (o[4] == 0) | (o[4] == 6)
    assert (o[4] == 0).sum() >= 8 and _same(h[2][rep], o[2][rep]) and _same(h[3][rep], o[3][rep])


def test_composition_with_the_optimal_rule_is_fixture_g14(golden_dir, rule="numpy"):
    """option on: the same composition with `optimal_cpts` for the barcode tail == the reference's own code around a stand-in
    for ruptures.KernelCPD (tests/golden/make_golden_optimal.py)"""
    g = np.load(os.path.join(golden_dir, "g14_refine_optimal.npz"))
    assert int(g["n"]) == 12
    sts, tags = [], []
    for k in range(int(g["n"])):
        seg, ref = params_from(g, k)
        a_s, a_e = (int(v) for v in g[f"args_{k}"])
        st, fpt, dwell, stats, idx = oc.refine_one(g[f"row_{k}"], a_s, a_e, seg, ref, g["consensus"], optimal=True, rule=rule)
        tag = str(g[f"tag_{k}"])
        assert st == int(g[f"status_{k}"]), (k, tag, st)
        assert _same(fpt, g[f"fpt_{k}"]) and _same(dwell, g[f"dwell_{k}"]), (k, tag)
        assert _same(stats, g[f"stats_{k}"]) and _same(idx, g[f"idx_{k}"]), (k, tag)
        sts.append(st)
        tags.append(tag)
    assert sts[tags.index("infeasible_tail")] == 3 and sts[tags.index("late_consensus")] == 6
    assert sts[tags.index("shrunk_width")] == 0 and sts.count(0) >= 8


def test_composition_through_the_c_statement_is_fixture_g14(golden_dir):
    """the same twelve cases, every array, with the oracle's wdx_oracle_optimal_cpts evaluating the tail"""
    test_composition_with_the_optimal_rule_is_fixture_g14(golden_dir, rule="c")


def _spc(optimal):
    return NS(sig_extract=NS(padding=100, normalization="none"), core=NS(sig_norm_outlier_thresh=5.0),
              segmentation=NS(min_obs_per_base=9, running_stat_width=18, num_events=120, accept_less_cpts=False,
                              normalization="mean", barcode_num_events=[25, 25], consensus_refinement=True,
                              consensus_model="rna004_130bps_v1_0", consensus_subseq_match_normalization="mean",
                              consensus_subseq_match_penalty=1.5, consensus_subseq_match_psi=[5, 0, 40, 0],
                              consensus_subseq_match_ub_start=18, consensus_subseq_match_lb_end=69,
                              consensus_subseq_match_ub_end=97, refinement_optimal_cpts=optimal))


def test_from_spc_and_constructor_rules():
    q = np.linspace(-1, 1, 84)
    assert sig_proc.RefineParams().optimal_cpts is False and sig_proc.RefineParams(query=q, optimal_cpts=True).optimal_cpts
    # the default refusal is what it was
    with pytest.raises(NotImplementedError, match=r"refinement_optimal_cpts \(ruptures KernelCPD\) is not offered by the HIP engine"):
        sig_proc.RefineParams.from_spc(_spc(True), q)
    with pytest.raises(NotImplementedError, match="refinement_optimal_cpts"):
        sig_proc.detect_results_to_fpt_batch(np.zeros((1, 3000), np.float32), _spc(True),
                                             [sig_proc.DetectResults(True, "", 100, 2900)], consensus_query=q)
    # with the keyword the field follows the configuration
    assert sig_proc.RefineParams.from_spc(_spc(True), q, optimal_cpts=True).optimal_cpts is True
    assert sig_proc.RefineParams.from_spc(_spc(False), q, optimal_cpts=True).optimal_cpts is False
    assert sig_proc.RefineParams.from_spc(_spc(False), q).optimal_cpts is False
    # not a field of wdx_refine_params
    on, off = sig_proc.RefineParams(query=q, optimal_cpts=True).to_c(), sig_proc.RefineParams(query=q).to_c()
    assert [n for n, _ in on._fields_] == [n for n, _ in off._fields_] and "optimal_cpts" not in [n for n, _ in on._fields_]
    assert all(getattr(on, n) == getattr(off, n) for n, _ in on._fields_ if n not in ("query", "psi"))
    # long_windows together with optimal_cpts: refused before any context exists
    rp = sig_proc.RefineParams(query=q, optimal_cpts=True)
    from warpdemux_amd import feeder, live, pipeline

    made = []
    real = _lib.Context

    class Spy(real):
        def __init__(self, *a, **kw):
            made.append(1)
            raise AssertionError("a context was created")

    _lib.Context = Spy
    try:
        for build in (lambda: pipeline.MinibatchPipeline(refs=None, refine=rp, long_windows=True),
                      lambda: live.LiveDemux(refs=np.zeros((2, 25)), refine=rp, long_windows=True),
                      lambda: feeder.Feeder(refs=None, refine=rp, long_windows=True),
                      lambda: sig_proc.fingerprint_refine_batch(np.zeros((1, 3000), np.float32), [100], [2900],
                                                                sig_proc.SegParams(), rp, long_windows=True)):
            with pytest.raises(ValueError, match="optimal_cpts and long_windows"):
                build()
    finally:
        _lib.Context = real
    assert not made


def test_constants_follow_the_header():
    hdr = open(os.path.join(ROOT, "include", "wdx.h")).read()
    assert re.search(r"^#define\s+WDX_OPT_REFINE_OPTIMAL_CPTS\s+(\d+)", hdr, flags=re.M).group(1) == str(_lib.OPT_REFINE_OPTIMAL_CPTS) == "23"
    assert re.search(r"^#define\s+WDX_K_REFINE_OPTIMAL\s+(\d+)", hdr, flags=re.M).group(1) == str(_lib.K_REFINE_OPTIMAL)
    assert "wdx_selftest_optimal_cpts_dev" in _lib.EXPORTS and re.search(r"\bwdx_selftest_optimal_cpts_dev\(", hdr)
    assert re.search(r"^#define\s+WDX_ABI_VERSION\s+(\d+)", hdr, flags=re.M).group(1) == str(_lib.ABI_VERSION)


def test_against_ruptures_when_it_is_installed():
    """Parity with the library itself is unpinned; where it imports: both answers are feasible and their exact costs differ
    by no more than the rounding bound.  The share of identical change-point sets is reported."""
    rpt = pytest.importorskip("ruptures")
    rng = np.random.default_rng(5)
    same = 0
    for _ in range(50):
        N, m, B = int(rng.integers(30, 200)), int(rng.integers(1, 6)), int(rng.integers(1, 5))
        x = rng.normal(size=N) + np.repeat(rng.normal(0, 3, 10), (N + 9) // 10)[:N]
        mine = oc.optimal_cpts(x, B, m)
        theirs = np.array([0] + list(rpt.KernelCPD(kernel="linear", min_size=m).fit(x.reshape(-1, 1)).predict(n_bkps=B)))
        assert np.diff(mine).min() >= m and np.diff(theirs).min() >= m and theirs[-1] == N
        assert abs(float(oc.exact_cost(x, mine) - oc.exact_cost(x, theirs))) <= oc.rounding_bound(x)
        same += int(np.array_equal(mine, theirs))
    print("identical change-point sets: %d of 50" % same)
