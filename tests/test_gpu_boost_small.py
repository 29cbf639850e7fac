"""The tree-parallel boost kernel for minibatch-sized batches (wdx_boost.hip: boost_small_kernel; WDX_OPT_BOOST_KERNEL)
against the lane-per-read kernel and the NumPy restatement (tests/helpers/boost_ref.py).

Per case the model runs under option 1 (lane-per-read only) and option 2 (tree-parallel only) through
wdx_boost_predict_dev: raw, prob, pred and conf must be the same bits (NaN by position), raw must equal
`boost_ref.raw_scores` exactly, and prob / conf / pred pass `boost_ref.check_outputs` -- the contract of
tests/test_gpu_boost.py, nothing looser.  Sizes sit on the kernel's boundaries: R = WDX_BOOST_SMALL_READS reads per
workgroup, CH = WDX_BOOST_TREE_CHUNK trees per chunk."""
import functools

import numpy as np
import pytest

from helpers import boost_ref
from warpdemux_amd import _lib, models, sig_proc

pytestmark = pytest.mark.gpu

R, CH = _lib.BOOST_SMALL_READS, _lib.BOOST_TREE_CHUNK
MIXED = (0, 1, 6, 10, 3)
SHALLOW = (0, 1, 2)
# (n, trees, depth spec, dim, features, NaN treatment, extra); every n, tree count, depth spec, dim and feature count of the
# list below occurs, the big tree counts with depth <= 2 and depth 16 with dim <= 2 and <= 3 trees
CASES = [
    (1, 1, 0, 1, 1, "AsIs", None),
    (R - 1, 63, 1, 3, 25, "AsTrue", None),
    (R, 65, 6, 4, 25, "AsFalse", None),
    (R + 1, CH - 1, 2, 4, 64, "AsTrue", None),
    (5 * R + 3, CH, 2, 8, 25, "AsIs", None),
    (R + 1, CH + 1, 1, 16, 25, "AsTrue", None),
    (5 * R + 3, 2 * CH + 7, SHALLOW, 1, 254, "AsFalse", None),
    (R, 3, 16, 2, 25, "AsTrue", None),
    (R - 1, 2, (16, 3), 1, 254, "AsIs", None),
    (5 * R + 3, 65, MIXED, 4, 64, "AsTrue", None),
    (5 * R + 3, 63, 6, 16, 1, "AsIs", None),
    (1, CH + 1, 2, 3, 25, "AsTrue", None),
    (5 * R + 3, 65, 6, 4, 25, "AsTrue", "nonfinite"),
    (5 * R + 3, 65, 6, 4, 25, "AsIs", "nonfinite"),
    (R + 1, 65, MIXED, 8, 25, "mixed", "nonfinite"),
    (5 * R + 3, 63, 6, 4, 25, "AsFalse", "borders"),
    (5 * R + 3, 65, 6, 4, 25, "AsTrue", "failed"),
    (R, 2 * CH + 7, SHALLOW, 3, 64, "AsIs", "failed"),
]
assert {c[0] for c in CASES} == {1, R - 1, R, R + 1, 5 * R + 3}
assert {c[1] for c in CASES} >= {1, 63, 65, CH - 1, CH, CH + 1, 2 * CH + 7}
assert {c[3] for c in CASES} >= {1, 3, 4, 8, 16} and {c[4] for c in CASES} == {1, 25, 64, 254}


def _case_id(i):
    n, t, d, dim, f, nan, extra = CASES[i]
    ds = "x".join(map(str, d)) if isinstance(d, tuple) else str(d)
    return f"n{n}-{t}t-d{ds}-dim{dim}-f{f}-{nan}" + (f"-{extra}" if extra else "")


@functools.lru_cache(maxsize=None)
def _engine():
    from warpdemux_amd.engine import DemuxEngine

    return DemuxEngine(np.zeros((1, 25)), 15, 0.1, sig_proc.SegParams(barcode_num_events=25))


def _labels(k, seed):
    return {i: int(v) for i, v in enumerate(np.random.default_rng(seed).permutation(k) * 3 + 1)}


def _device_model(m, label_mapper, thresholds=None):
    trees = [(f, b, [m.nan_treatment[i] == "AsTrue" for i in f], lv) for f, b, lv in m.trees]
    return models.Fpt_Boost(trees, m.n_features, m.scale, m.bias, label_mapper, thresholds)


@functools.lru_cache(maxsize=None)
def _case(i):
    """model, rows, status, label map, thresholds and the restatement's figures of CASES[i]: computed once, never modified"""
    n, n_trees, depth, dim, n_features, nan, extra = CASES[i]
    treat = ([boost_ref.NAN_TREATMENTS[j % 3] for j in range(n_features)] if nan == "mixed" else [nan] * n_features)
    m = boost_ref.random_model(n_trees, depth, dim, n_features, seed=500 + i, nan_treatment=treat)
    X = boost_ref.random_inputs(m, n, seed=600 + i)
    rng = np.random.default_rng(700 + i)
    X[rng.random(X.shape) < 0.02] = np.nan                         # a few NaN features in every case
    if extra == "nonfinite":
        X[rng.random(X.shape) < 0.05] = np.nan
        X[rng.random(X.shape) < 0.05] = np.inf
        X[rng.random(X.shape) < 0.05] = -np.inf
        assert np.isnan(X).any() and np.isposinf(X).any() and np.isneginf(X).any()
    hits = 0
    if extra == "borders":                                         # values equal to a border: the compare is false
        for t, (feat, border, _) in enumerate(m.trees):
            for f, b in zip(feat, border):
                X[(7 * t + int(f)) % n, f] = float(b)
                hits += 1
        assert hits > 100
    status = None
    if extra == "failed":
        status = np.zeros(n, dtype=np.int32)
        status[[0, n - 1]] = (3, 6)
        if n > R:
            status[R:2 * R] = 1 + np.arange(R) % 6                 # a workgroup whose reads all failed
            status[3 * R + 5] = 2
    thr = np.random.default_rng(i).uniform(0.05, 0.6, m.k) if i % 2 else None
    c = boost_ref.contract(m, X, thr)
    X.setflags(write=False)
    return m, X, status, _labels(m.k, i), thr, c


def _run(eng, option, X, status):
    import torch

    eng.ctx.set_option(_lib.OPT_BOOST_KERNEL, option)
    try:
        Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(eng.tdev)
        sd = None if status is None else torch.from_numpy(status).to(eng.tdev)
        prob, pred, conf, raw = eng.boost_predict(Xd, sd, want_raw=True)
        return raw.cpu().numpy(), prob.cpu().numpy(), pred.cpu().numpy(), conf.cpu().numpy()
    finally:
        eng.ctx.set_option(_lib.OPT_BOOST_KERNEL, 0)


@pytest.mark.parametrize("i", range(len(CASES)), ids=_case_id)
def test_tree_parallel_kernel_gives_the_bits_of_the_lane_per_read_kernel(i):
    m, X, status, lm, thr, c = _case(i)
    eng = _engine()
    eng.set_boost(_device_model(m, lm, thr))
    lane = _run(eng, 1, X, status)
    tree = _run(eng, 2, X, status)
    for name, a, b in zip(("raw", "prob", "pred", "conf"), lane, tree):
        same = a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=name != "pred")
        print(f"{_case_id(i)}: {name} lane-per-read == tree-parallel: {same}")
        assert same, name
    ok = np.ones(len(X), dtype=bool) if status is None else status == 0
    raw, prob, pred, conf = tree
    assert raw.shape == (len(X), m.dim) and prob.shape == (len(X), m.k)
    assert np.array_equal(raw[ok], c["raw"][ok]), f"max |raw - restatement| = {np.abs(raw[ok] - c['raw'][ok]).max():.3g}"
    assert (pred[~ok] == -1).all() and np.isnan(raw[~ok]).all() and np.isnan(prob[~ok]).all() and np.isnan(conf[~ok]).all()
    pred_ref, _ = boost_ref.process_probs(c["p64"], lm, thr)
    sub = {k: (v[ok] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    err, bad = boost_ref.check_outputs(sub, prob[ok], conf[ok], pred[ok], pred_ref[ok])
    print(f"{_case_id(i)}: E_ref {c['e_ref']:.3g} T {c['T']:.3g} gpu err {err:.3g} close {int(c['close'].sum())}/{len(X)}")
    assert not bad, bad


def test_negative_control_under_the_tree_parallel_kernel():
    """one leaf value moved until the exact outputs move by >= 10 T: the tree-parallel kernel's result of the perturbed model
    fails the check against the unperturbed figures, and its raw scores are no longer the restatement's"""
    m = boost_ref.random_model(CH + 1, 2, 4, 25, seed=31)
    X = boost_ref.random_inputs(m, 5 * R + 3, seed=32)
    lm = _labels(4, 3)
    c = boost_ref.contract(m, X)
    m2, moved = boost_ref.perturb_leaf(m, X, c["T"])
    pred_ref, _ = boost_ref.process_probs(c["p64"], lm)
    eng = _engine()
    eng.set_boost(_device_model(m2, lm))
    raw, prob, pred, conf = _run(eng, 2, X, None)
    err, bad = boost_ref.check_outputs(c, prob, conf, pred, pred_ref)
    print(f"negative control: moved {moved:.3g}, T {c['T']:.3g}, gpu err {err:.3g}")
    assert moved >= 10 * c["T"] and bad and not np.array_equal(raw, c["raw"])
    eng.set_boost(_device_model(m, lm))
    raw, prob, pred, conf = _run(eng, 2, X, None)
    assert np.array_equal(raw, c["raw"]) and not boost_ref.check_outputs(c, prob, conf, pred, pred_ref)[1]


def test_dispatch_and_kernel_accounting(capfd):
    """WDX_OPT_DEBUG_OCCUPANCY names the kernel of every boost launch: options 1 and 2 force theirs at any size, the default
    takes the tree-parallel kernel up to WDX_BOOST_SMALL_MAX_READS reads and not one read beyond (asserted once that
    constant is not 0); WDX_K_BOOST counts whichever ran."""
    import ctypes as C

    m, X, _, lm, thr, _c = _case(2)
    eng = _engine()
    eng.set_boost(_device_model(m, lm, thr))
    L, h = _lib.load(), eng.ctx.handle

    def which(option, n):
        rows = np.resize(X, (n, X.shape[1]))
        capfd.readouterr()
        eng.ctx.set_option(_lib.OPT_DEBUG_OCCUPANCY, 1)
        try:
            _run(eng, option, rows, None)
        finally:
            eng.ctx.set_option(_lib.OPT_DEBUG_OCCUPANCY, 0)
        lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("wdx boost:")]
        assert len(lines) == 1 and f"{n} reads" in lines[0], lines
        return lines[0].split()[2]

    _lib.check(L.wdx_kernel_timing(h, 1))
    try:
        _lib.check(L.wdx_kernel_time_reset(h))
        assert which(1, R) == "lane-per-read" and which(2, 5 * R + 3) == "tree-parallel" and which(2, 1000) == "tree-parallel"
        ms, launches = C.c_double(0), C.c_int64(0)
        _lib.check(L.wdx_kernel_time(h, _lib.K_BOOST, C.byref(ms), C.byref(launches)))
        assert launches.value == 3 and ms.value > 0
    finally:
        _lib.check(L.wdx_kernel_timing(h, 0))
    n_small = _lib.BOOST_SMALL_MAX_READS
    assert which(0, n_small + 1) == "lane-per-read"
    if n_small > 0:
        assert which(0, n_small) == "tree-parallel" and which(0, 1) == "tree-parallel"
