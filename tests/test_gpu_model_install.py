"""The one install path of the three resident classifier models (wdx_classify.hip: install; include/wdx.h, "Resident
models"): every wdx_*_set_model puts the model's image into a block of its own, binds the kernels' record to that block only
after the swap, and counts the change.  One test per kind, 64 reads through the kind's device-resident entry:

    set A, predict | set B (a model of another size), predict | set A again, predict

The first and the third outputs are the same bits (nothing of B is left: neither a pointer into its block nor, for the SVM,
the references gathered in B's support-vector order -- the fused route of wdx_demux_svm_dev rebuilds them at every change of
the model), and the second equals, bit for bit, a fresh context that only ever saw B.  A and B give different answers, and
most reads succeed, or the comparison would hold for any model.

The minibatch path has no WANT bit for the MLP (WDX_WANT_SVM and WDX_WANT_BOOST are the two tails a slot serves), so case (E)
of tests/test_gpu_streams.py cannot hold wdx_mlp_set_model behind a minibatch in flight; its behind-pending-work case (C)
does, and the setter now shares every line of its waiting with the two that (E) holds."""
import functools

import numpy as np
import pytest

from helpers import boost_ref, mlp_ref, svm_ref
from helpers import refine_inputs as ri
from oracle import wdx_oracle as orc
from warpdemux_amd import models, sig_proc

pytestmark = pytest.mark.gpu

K, N_READS, N_REFS, WINDOW, PENALTY = 25, 64, 12, 15, 0.1
STRIDE = 6208     # rows of tests/helpers/refine_inputs.py (at most 6 200 samples), a multiple of 8


@functools.lru_cache(maxsize=None)
def _inputs():
    """64 reads of tests/helpers/refine_inputs.py as strided float32 rows, and N_REFS of their own fingerprints (the CPU
    oracle's), a little off, as the reference set"""
    b = ri.batch(1)
    rows = np.full((N_READS, STRIDE), np.nan, dtype=np.float32)
    rows[:, :b["rows"].shape[1]] = b["rows"][:N_READS]
    a_s, a_e, ok = b["a_s"][:N_READS].copy(), b["a_e"][:N_READS].copy(), b["ok"][:N_READS].copy()
    win = np.minimum(a_e.astype(np.int64) + ri.PADDING, STRIDE) - np.maximum(a_s.astype(np.int64) - ri.PADDING, 0)
    fpt, _, _, status = orc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], orc.SegParams(barcode_num_events=K, **ri.SEG), b["ok"])
    refs = np.ascontiguousarray(fpt[status == 0][:N_REFS]) + 0.01
    assert refs.shape == (N_REFS, K)
    return rows, a_s, a_e, ok, int(win[ok != 0].max()), refs


def _engine():
    from warpdemux_amd.engine import DemuxEngine

    return DemuxEngine(_inputs()[5], WINDOW, PENALTY, sig_proc.SegParams(barcode_num_events=K, **ri.SEG))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g), _bits(w))
                                         for g, w in zip(got, want))


def _a_b_a(kind, model_a, model_b, call):
    """call(engine, device tensors) -> output tensors whose element 3 is the status; returns the three outputs and B's alone"""
    import torch

    rows, a_s, a_e, ok, max_len, _ = _inputs()
    outs = []
    for sequence in ((model_a, model_b, model_a), (model_b,)):
        eng = _engine()
        try:
            t = [torch.from_numpy(x).to(eng.tdev) for x in (rows, a_s, a_e, ok)]
            for m in sequence:
                getattr(eng, "set_" + kind)(m)
                outs.append([o.cpu().numpy() for o in call(eng, *t, max_len) if o is not None])
        finally:
            eng.close()
    first, second, third, b_alone = outs
    status = first[3]
    assert (status == 0).sum() * 2 > N_READS, np.bincount(status)
    assert not _same(first[:3], second[:3]), "A and B answer alike"
    assert _same(first, third), "A after B is not A"
    assert _same(second, b_alone), "B after A is not B"


def test_svm_a_b_a_through_the_fused_route():
    """wdx_demux_svm_dev without distances: the fused DTW + SVM route, whose gathered references follow the model"""
    refs = _inputs()[5]
    a = svm_ref.synth_model(3, seed=5, n_support=[2, 1, 3], n_extra=6, thresholds=True, gamma=0.02)
    b = svm_ref.synth_model(4, seed=6, n_support=[3, 2, 1, 4], n_extra=2, thresholds=False, gamma=0.03, pwr_dist=2)
    assert a.n_train == b.n_train == N_REFS
    _a_b_a("svm", a.to_dtw_svm(refs), b.to_dtw_svm(refs),
           lambda e, rows, a_s, a_e, ok, ml: e.demux_svm(rows, a_s, a_e, stride=STRIDE, max_len=ml, ok=ok))


def test_mlp_a_b_a():
    refs = _inputs()[5]

    def model(hidden, k, dtype, act, seed, thr):
        est = mlp_ref.random_mlp(N_REFS, hidden, k, dtype, act, seed=seed)
        return models.from_reference(mlp_ref.DTW_MLP(est, refs, {i: 3 * i + 1 for i in range(k)}, thr, window=WINDOW, penalty=PENALTY))

    _a_b_a("mlp", model((16,), 5, np.float32, "relu", 9, np.linspace(0.05, 0.3, 5)), model((33, 20), 3, np.float64, "tanh", 10, None),
           lambda e, rows, a_s, a_e, ok, ml: e.demux_mlp(rows, a_s, a_e, stride=STRIDE, max_len=ml, ok=ok))


def test_boost_a_b_a():
    def model(n_trees, depths, dim, seed, thr):
        bm = boost_ref.random_model(n_trees, depths, dim, K, seed=seed)
        trees = [(f, bo, [bm.nan_treatment[i] == "AsTrue" for i in f], lv) for f, bo, lv in bm.trees]
        return models.Fpt_Boost(trees, bm.n_features, bm.scale, bm.bias, {i: 2 * i + 1 for i in range(max(dim, 2))}, thr)

    def call(e, rows, a_s, a_e, ok, ml):
        prob, pred, conf, status, _, fpt, raw = e.demux_boost(rows, a_s, a_e, None, stride=STRIDE, max_len=ml, ok=ok, want_fpt=True,
                                                              want_raw=True)
        return prob, pred, conf, status, fpt, raw

    _a_b_a("boost", model(2, (1, 0), 4, 81, np.array([0.05, 0.2, 0.1, 0.3])), model(33, (0, 1, 6, 3), 1, 82, None), call)
