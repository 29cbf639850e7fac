"""Optimal change-points of the consensus refinement (WDX_OPT_REFINE_OPTIMAL_CPTS), the parts that need no GPU: the NumPy
restatement of the rule (tests/helpers/optimal_cpts.py) against brute force in exact arithmetic, its ties, the refinement
branch composed of the oracle's primitives against the oracle (peak rule) and against fixture g14 (optimal rule), and the
constructor rules of the Python layer."""
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


def test_composition_with_the_optimal_rule_is_fixture_g14(golden_dir):
    """option on: the same composition with `optimal_cpts` for the barcode tail == the reference's own code around a stand-in
    for ruptures.KernelCPD (tests/golden/make_golden_optimal.py)"""
    g = np.load(os.path.join(golden_dir, "g14_refine_optimal.npz"))
    assert int(g["n"]) == 12
    sts, tags = [], []
    for k in range(int(g["n"])):
        seg, ref = params_from(g, k)
        a_s, a_e = (int(v) for v in g[f"args_{k}"])
        st, fpt, dwell, stats, idx = oc.refine_one(g[f"row_{k}"], a_s, a_e, seg, ref, g["consensus"], optimal=True)
        tag = str(g[f"tag_{k}"])
        assert st == int(g[f"status_{k}"]), (k, tag, st)
        assert _same(fpt, g[f"fpt_{k}"]) and _same(dwell, g[f"dwell_{k}"]), (k, tag)
        assert _same(stats, g[f"stats_{k}"]) and _same(idx, g[f"idx_{k}"]), (k, tag)
        sts.append(st)
        tags.append(tag)
    assert sts[tags.index("infeasible_tail")] == 3 and sts[tags.index("late_consensus")] == 6
    assert sts[tags.index("shrunk_width")] == 0 and sts.count(0) >= 8


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
