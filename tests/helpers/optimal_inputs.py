"""Inputs of tests/test_gpu_optimal_cpts.py: fixture g14 (tests/golden/make_golden_optimal.py) case by case, and its nine
reads that share the tRNA parameter set as ONE minibatch with the fixture's outputs stacked beside it."""
import os

import numpy as np

from test_oracle_refine import params_from
from warpdemux_amd import sig_proc

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(a.shape == b.shape and np.array_equal(a, b, equal_nan=True))


def g14():
    return np.load(os.path.join(GOLDEN, "g14_refine_optimal.npz"))


def g14_cases():
    """[(k, tag, row, a_start, a_end, SegParams, RefineParams with optimal_cpts, expected dict)]"""
    g = g14()
    out = []
    for k in range(int(g["n"])):
        seg, ref = params_from(g, k)
        a_s, a_e = (int(v) for v in g[f"args_{k}"])
        exp = dict(status=np.int32(g[f"status_{k}"]), fpt=g[f"fpt_{k}"], dwell=g[f"dwell_{k}"], stats=g[f"stats_{k}"],
                   refine_idx=g[f"idx_{k}"].astype(np.int32))
        out.append((k, str(g[f"tag_{k}"]), g[f"row_{k}"], a_s, a_e, seg, ref, exp))
    return out


def g14_minibatch():
    """the cases whose parameters are those of case 0 (embedded, late consensus, shrunk width, infeasible tail): rows (n,
    stride) float32 with a NaN tail, a_s / a_e, params / refine (optimal_cpts=True), and the fixture's status / fpt / dwell /
    stats / refine_idx stacked"""
    g = g14()
    cases = g14_cases()
    seg0, ref0 = cases[0][5], cases[0][6]
    pick = [c for c in cases if c[5] == seg0 and c[6] == ref0]
    tags = [c[1] for c in pick]
    assert len(pick) == 9 and {"embedded", "late_consensus", "shrunk_width", "infeasible_tail"} <= set(tags), tags
    stride = max(c[2].size for c in pick) + 64
    rows = np.full((len(pick), stride), np.nan, dtype=np.float32)
    for i, c in enumerate(pick):
        rows[i, : c[2].size] = c[2]
    mb = dict(rows=rows, a_s=np.array([c[3] for c in pick], dtype=np.int32), a_e=np.array([c[4] for c in pick], dtype=np.int32),
              tags=tags, seg=seg0, ref=ref0, consensus=g["consensus"], params=sig_proc.SegParams(**seg0),
              refine=sig_proc.RefineParams(query=g["consensus"], optimal_cpts=True, **ref0),
              refine_off=sig_proc.RefineParams(query=g["consensus"], **ref0))
    mb["status"] = np.array([c[7]["status"] for c in pick], dtype=np.int32)
    for name in ("fpt", "dwell", "stats", "refine_idx"):
        mb[name] = np.stack([c[7][name] for c in pick])
    return mb
