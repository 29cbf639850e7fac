"""Consensus refinement on adapter windows of 16 385 .. 65 536 samples: the oracle, which has no window limit, against fixture
g13 -- the REFERENCE's own detect_results_to_fpt with consensus_refinement = True on such windows
(tests/golden/make_golden_refine_long.py; the dtaidistance call inside `_get_subseq_match` is g8's pure-Python stand-in, so the
subsequence match stays parity-unpinned as in tests/test_oracle_refine.py, everything around it is pinned)."""
import numpy as np

from helpers import refine_long_inputs as rl
from oracle import wdx_oracle as orc


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_g13_refinement_of_long_windows_bit_for_bit():
    g = rl.g13()
    tags, lengths = set(), set()
    for k in range(int(g["n"])):
        seg, ref, clip64 = rl.params_from(g, k)
        row = g[f"row_{k}"]
        a_s, a_e = (int(v) for v in g[f"args_{k}"])
        fpt, dwell, stats, idx, status = orc.fingerprint_refine_batch(
            row.reshape(1, -1), [a_s], [a_e], orc.SegParams(clip_bounds_f64=clip64, **seg),
            orc.RefineParams(query=g["consensus"], **ref))
        st, tag = int(g[f"status_{k}"]), str(g[f"tag_{k}"])
        assert status[0] == st, f"case {k} ({tag}): status {status[0]} != {st}"
        assert _same(stats[0], g[f"stats_{k}"]), f"case {k} ({tag}) stats"
        assert _same(idx[0], g[f"idx_{k}"].astype(np.int32)), f"case {k} ({tag}) query start / end, barcode start"
        assert _same(fpt[0], g[f"fpt_{k}"]), f"case {k} ({tag}) fpt"
        assert _same(dwell[0], g[f"dwell_{k}"]), f"case {k} ({tag}) dwell"
        tags.add(tag)
        lengths.add(row.size)
    assert {16385, 20000, 32769, 49152, 65536} <= lengths
    assert {"no_consensus_20000", "clip64_32769", "embedded_65536"} <= tags
    sts = [int(g[f"status_{k}"]) for k in range(int(g["n"]))]
    assert sts.count(0) >= 6 and sts.count(6) >= 1
