"""Nearest-reference calls with reference labels, margin and rejection -- everything that needs no GPU.

(1) the header's new prototypes are exported by the built library, the ABI version stays 4;
(2) tests/helpers/nearest_rule.py -- the NumPy statement of the rule every GPU test compares against -- is itself pinned by
    hand-worked rows;
(3) nearest_plan (warpdemux_amd/csrc/wdx_dtw_plan.h): the "rule fused / rule after / block buffer" decision for the shapes
    tests/test_gpu_nearest.py runs, and its invariants over a sweep (tests/host/nearest_plan_check.cpp, system compiler, address
    and undefined-behaviour sanitizers, stand-alone);
(4) the Python layer's argument refusals."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from warpdemux_amd import _lib, _nearest
from warpdemux_amd import parallel_distances as pdist

from helpers.nearest_rule import QNAN, nearest_rule, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
NEW = ("wdx_nearest_dev", "wdx_demux_nearest_dev", "wdx_dtw_nearest")
inf = np.float32(np.inf)
nan = np.float32(np.nan)


def test_new_prototypes_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "wdx.h")).read()
    assert re.search(r"#define WDX_ABI_VERSION 4\b", hdr) and _lib.ABI_VERSION == 4
    L = _lib.load()
    assert L.wdx_abi_version() == 4
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    # the argument lists bound in _lib.py are as long as the header's
    for name in NEW:
        args = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(getattr(L, name).argtypes) == args.count(",") + 1, name


def _f32(*rows):
    return np.array(rows, dtype=np.float32)


def _up(x):
    return np.nextafter(np.float32(x), inf)


# (row of distances, labels, keyword arguments) -> (call, d1, d2), each worked out by hand from the rule's statement
HAND_ROWS = [
    # plain: nearest is column 1 (label 1), nearest of another label is column 2
    ([3, 1, 2, 5], [0, 1, 0, 1], {}, (1, 1, 2)),
    # tie across labels: margin exactly 0, the call is the smaller column's label
    ([2, 1, 1, 4], [0, 1, 2, 0], {}, (1, 1, 1)),
    ([2, 1, 1, 4], [0, 2, 1, 0], {}, (2, 1, 1)),
    # tie within a label: d2 skips the twin
    ([1, 1, 3, 2], [0, 0, 1, 2], {}, (0, 1, 2)),
    # the best label's other references never count for d2, however close
    ([1, 1.5, 1.25, 9], [4, 4, 4, 0], {"n_labels": 5}, (4, 1, 9)),
    # a NaN column wins outright: d1 = d2 = NaN, rejected whatever the thresholds
    ([1, nan, 0.5], [0, 1, 2], {}, (-1, nan, nan)),
    ([nan, nan, 0.5], [0, 1, 2], {"min_margin": -inf}, (-1, nan, nan)),
    # all +inf: argmin is column 0, d1 = d2 = inf; accepted without thresholds, margin NaN rejects under any min_margin
    ([inf, inf, inf], [2, 1, 0], {}, (2, inf, inf)),
    ([inf, inf, inf], [2, 1, 0], {"min_margin": -inf}, (-1, inf, inf)),
    ([inf, inf, inf], [2, 1, 0], {"max_dist": inf}, (2, inf, inf)),
    # one label only: d2 = +inf, the margin is +inf
    ([4, 2, 3], [0, 0, 0], {"n_labels": 1, "min_margin": 1e30}, (0, 2, inf)),
    # identity labels
    ([4, 2, 3], None, {}, (1, 2, 3)),
    # a threshold exactly equal to the margin accepts, one float32 ulp above it rejects
    ([1.5, 4.75], [0, 1], {"min_margin": 3.25}, (0, 1.5, 4.75)),
    ([1.5, 4.75], [0, 1], {"min_margin": _up(3.25)}, (-1, 1.5, 4.75)),
    # max_dist: equal accepts, one ulp below d1 rejects; thresholds are per label (label 1's would reject)
    ([1.5, 4.75], [0, 1], {"max_dist": [1.5, 0.0]}, (0, 1.5, 4.75)),
    ([1.5, 4.75], [0, 1], {"max_dist": [np.nextafter(np.float32(1.5), -inf), 9.0]}, (-1, 1.5, 4.75)),
    # a NaN threshold rejects (the comparisons are written negated)
    ([1.5, 4.75], [0, 1], {"min_margin": nan}, (-1, 1.5, 4.75)),
]


@pytest.mark.parametrize("k", range(len(HAND_ROWS)))
def test_helper_on_hand_worked_rows(k):
    d, g, kw, (call, d1, d2) = HAND_ROWS[k]
    c, best, counts = nearest_rule(_f32(d), g, **kw)
    G = len(counts) - 1
    assert c.dtype == np.int32 and best.dtype == np.float32 and counts.dtype == np.int64
    assert int(c[0]) == call
    assert same_bits(best, _f32([d1, d2])) or (np.isnan(d1) and same_bits(best, np.array([[QNAN, QNAN]], dtype=np.float32)))
    want = np.zeros(G + 1, dtype=np.int64)
    want[call if call >= 0 else G] = 1
    assert np.array_equal(counts, want)


def test_helper_status_and_counts():
    D = _f32([3, 1, 2], [1, 2, 3], [2, 2, 1], [5, 4, 6])
    call, best, counts = nearest_rule(D, [0, 1, 1], n_labels=3, status=np.array([0, 7, 0, 0]), max_dist=[9, 3, 9])
    assert call.tolist() == [1, -1, 1, -1]          # row 1 failed, row 3 is beyond label 1's max_dist
    assert same_bits(best[1], np.array([QNAN, QNAN], dtype=np.float32)) and best[0].tolist() == [1, 3] and best[3].tolist() == [4, 5]
    assert counts.tolist() == [0, 2, 0, 2] and counts.sum() == 4
    # identity labels, no thresholds: the call is the argmin wherever the row has no NaN
    rng = np.random.default_rng(5)
    D = rng.random((200, 7), dtype=np.float32)
    D[::17, 3] = D[::17, 5]
    assert np.array_equal(nearest_rule(D)[0], np.argmin(D, axis=1).astype(np.int32))


# ---- the plan ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    out = str(tmp_path_factory.mktemp("nearest_plan") / "nearest_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "host", "nearest_plan_check.cpp"),
                           "-o", out])
    return out


FUSED, AFTER = 1, 2
# nX nY L window have_dist refs_any_inf entry no_wavefront no_short_dtw wide_dtw -> rule buffer block_rows family layout
# (the shapes of tests/test_gpu_nearest.py; worked out from the dispatch rule as DESIGN.md 4.3 states it: one lane walks all
# references from 2 048 waves of reads on when there are fewer than 32 of them, the wavefront kernel up to 16 384 pairs,
# references as lanes below a wave of reads, scratch rows beyond window 32, row-major from 8 192 reads on)
PLAN_CASES = [
    ((131072, 6, 25, 15, 1, 0, 0, 0, 0, 0), (FUSED, 0, 131072, _lib.DTW_SHORT, _lib.DTW_LAYOUT_ROW_MAJOR)),
    ((131072, 6, 25, 15, 0, 0, 0, 0, 0, 0), (FUSED, 0, 131072, _lib.DTW_SHORT, _lib.DTW_LAYOUT_ROW_MAJOR)),
    ((131072, 6, 40, 8, 0, 0, 0, 0, 0, 0), (FUSED, 0, 131072, _lib.DTW_BAND, _lib.DTW_LAYOUT_ROW_MAJOR)),
    ((131072, 6, 40, 15, 0, 0, 0, 0, 0, 0), (FUSED, 0, 131072, _lib.DTW_BAND, _lib.DTW_LAYOUT_ROW_MAJOR)),
    ((131072, 6, 40, 16, 0, 0, 0, 0, 0, 0), (FUSED, 0, 131072, _lib.DTW_BAND, _lib.DTW_LAYOUT_ROW_MAJOR)),
    ((131072, 6, 40, 32, 0, 0, 0, 0, 0, 0), (FUSED, 0, 131072, _lib.DTW_BAND, _lib.DTW_LAYOUT_ROW_MAJOR)),
    # a reference with an infinite sample: the matrix has to exist for the pass that settles equal infinities
    ((131072, 6, 25, 15, 0, 1, 0, 0, 0, 0), (AFTER, 1, 131072, _lib.DTW_SHORT, _lib.DTW_LAYOUT_ROW_MAJOR)),
    # read-minor: 4 096 reads are 64 waves, the references are split over grid.y -> after
    ((4096, 6, 25, 15, 0, 0, 0, 1, 0, 0), (AFTER, 1, 4096, _lib.DTW_SHORT, _lib.DTW_LAYOUT_READ_MINOR)),
    ((4096, 6, 25, 15, 0, 0, 1, 0, 0, 0), (AFTER, 1, 4096, _lib.DTW_SHORT, _lib.DTW_LAYOUT_READ_MINOR)),
    # read-minor and fused: a single reference is always walked by one lane
    ((4096, 1, 25, 15, 0, 0, 0, 1, 0, 0), (FUSED, 0, 4096, _lib.DTW_SHORT, _lib.DTW_LAYOUT_READ_MINOR)),
    ((1000, 40, 33, 15, 0, 0, 0, 0, 0, 0), (AFTER, 1, 1000, _lib.DTW_BAND, _lib.DTW_LAYOUT_READ_MINOR)),
    ((1000, 40, 33, 15, 1, 0, 0, 0, 0, 0), (AFTER, 0, 1000, _lib.DTW_BAND, _lib.DTW_LAYOUT_READ_MINOR)),
    ((8, 200, 25, 15, 0, 0, 0, 1, 0, 0), (AFTER, 1, 8, _lib.DTW_SHORT, _lib.DTW_LAYOUT_REFS_AS_LANES)),
    ((16, 10, 25, 15, 0, 0, 0, 0, 0, 0), (AFTER, 1, 16, _lib.DTW_WAVEFRONT, _lib.DTW_LAYOUT_ROW_MAJOR)),
    ((300, 5, 40, 0, 0, 0, 0, 0, 0, 0), (AFTER, 1, 300, _lib.DTW_SCRATCH, _lib.DTW_LAYOUT_READ_MINOR)),
    ((300, 5, 40, 0, 0, 0, 0, 0, 0, 1), (AFTER, 1, 300, _lib.DTW_WIDE, _lib.DTW_LAYOUT_READ_MINOR)),
    ((131072, 5, 40, 0, 0, 0, 0, 0, 0, 1), (FUSED, 0, 131072, _lib.DTW_WIDE, _lib.DTW_LAYOUT_ROW_MAJOR)),
    # the R2 shape without distances: 2 601 references x 4 bytes -> 9 664 rows (151 waves) per 96 MiB block
    ((200000, 2601, 25, 15, 0, 0, 0, 0, 0, 0), (AFTER, 1, 9664, _lib.DTW_SHORT, _lib.DTW_LAYOUT_ROW_MAJOR)),
    ((200, 2601, 25, 15, 0, 0, 0, 0, 0, 0), (AFTER, 1, 200, _lib.DTW_SHORT, _lib.DTW_LAYOUT_READ_MINOR)),
    # the fused raw-row path of the tests: 20 000 reads x 12 references
    ((20000, 12, 25, 15, 0, 0, 1, 0, 0, 0), (AFTER, 1, 20000, _lib.DTW_SHORT, _lib.DTW_LAYOUT_ROW_MAJOR)),
    # nothing to do / the fused entry's refusal
    ((0, 6, 25, 15, 0, 0, 0, 0, 0, 0), (0, 0, 0, _lib.DTW_NONE, 0)),
    ((10, 3, 110, 33, 0, 0, 1, 0, 0, 0), (0, 0, 0, _lib.DTW_NONE, 0)),
]


def test_plan_decisions_for_the_shapes_the_gpu_tests_use(exe):
    cases = "".join(" ".join(map(str, c)) + "\n" for c, _ in PLAN_CASES)
    run = subprocess.run([exe], input=cases.encode(), capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(int(v) for v in ln.split()) for ln in run.stdout.decode().splitlines()]
    assert len(got) == len(PLAN_CASES)
    for g, (c, (rule, buffer, block_rows, family, layout)) in zip(got, PLAN_CASES):
        assert g[:10] == c
        r, b, rows, nbytes, fam, _band_w, lay, fused, grid_y, unsupported, argmin_after = g[10:]
        assert (r, b, rows, fam, lay) == (rule, buffer, block_rows, family, layout), c
        assert fused == (rule == FUSED) and argmin_after == 0 and nbytes == (rows * c[1] * 4 if buffer else 0), c
        assert (grid_y == 1) if rule == FUSED else True
        assert unsupported == (c == (10, 3, 110, 33, 0, 0, 1, 0, 0, 0))
        assert nbytes <= 96 << 20


def test_plan_invariants_over_the_sweep(exe):
    run = subprocess.run([exe, "sweep"], capture_output=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    out = dict((ln.rsplit(" ", 1)[0], int(ln.rsplit(" ", 1)[1])) for ln in run.stdout.decode().splitlines())
    assert out["cases"] == 17 * 14 * 11 * 64
    assert out["rule 0"] + out["rule 1"] + out["rule 2"] == out["cases"]
    assert min(out["rule 0"], out["rule 1"], out["rule 2"]) > 1000


# ---- the Python layer's refusals ---------------------------------------------------------------------------------------------
def test_label_and_threshold_arguments_are_checked_on_the_host():
    ok, G = _nearest.host_labels(4, [0, 2, 2, 1], None)
    assert ok.dtype == np.int32 and G == 3
    assert _nearest.host_labels(4, None, None) == (None, 4)
    assert _nearest.host_labels(4, np.array([0, 0, 0, 0], dtype=np.uint8), 9)[1] == 9
    for bad_labels, n_labels in (([0, 1, 2], None),            # one label per reference
                                 ([[0, 1], [2, 3]], None),
                                 ([0.0, 1.0, 2.0, 3.0], None),   # an integer dtype
                                 ([True, False, True, False], None),
                                 ([0, 1, 2, 3], 3),              # every label below n_labels
                                 ([0, -1, 2, 3], None),
                                 (None, 3),                      # the identity needs n_labels = nY
                                 ([0, 1, 2, 3], 0),
                                 ([0, 1, 2, 3], 4.0),            # n_labels is an integer
                                 ([0, 1, 2, 3], True)):
        with pytest.raises(ValueError):
            _nearest.host_labels(4, bad_labels, n_labels)
    assert _nearest.host_threshold("min_margin", None, 3) is None
    assert _nearest.host_threshold("min_margin", 0.5, 3).tolist() == [0.5] * 3
    assert _nearest.host_threshold("max_dist", np.array([1, 2, 3]), 3).dtype == np.float32
    for bad in ([1.0, 2.0], [[1.0, 2.0, 3.0]], ["a", "b", "c"], [1j, 2j, 3j]):
        with pytest.raises(ValueError):
            _nearest.host_threshold("max_dist", bad, 3)


def test_nearest_label_refuses_before_it_needs_a_device():
    X, Y = np.zeros((3, 25)), np.zeros((4, 25))
    with pytest.raises(ValueError, match="one label per reference"):
        pdist.nearest_label(X, Y, labels=[0, 1, 2])
    with pytest.raises(ValueError, match="integer dtype"):
        pdist.nearest_label(X, Y, labels=np.array([0.0, 1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match="labels must lie in 0 .. 1"):
        pdist.nearest_label(X, Y, labels=[0, 1, 2, 3], n_labels=2)
    with pytest.raises(ValueError, match="n_labels"):
        pdist.nearest_label(X, Y, n_labels=3)
    with pytest.raises(ValueError, match="one threshold per label"):
        pdist.nearest_label(X, Y, labels=[0, 1, 1, 0], min_margin=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="same number of columns"):
        pdist.nearest_label(X, np.zeros((4, 24)))
    with pytest.raises(ValueError, match="2-dimensional"):
        pdist.nearest_label(np.zeros(25), Y)
