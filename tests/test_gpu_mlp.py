"""The DTW_MLP classifier tail on the device (wdx_mlp.hip) against scikit-learn and an exact forward pass.

Distances come from the engine's own DTW (wdx_dtw_matrix_dev), so only the tail is under test.  Accuracy contract per case
(tests/helpers/mlp_ref.py): E_ref = max |p_sklearn - p_exact|, T = 4 max(E_ref, u_w); |p - p_exact| <= T,
|conf - conf_exact| <= 2T, float32 models return float32 values, pred equals scikit-learn's + process_probs except on
close calls (at most 1 % of a case's reads).  Every case prints its figures before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import mlp_ref, svm_ref
from warpdemux_amd import _lib, models, sig_proc, synth

pytestmark = pytest.mark.gpu

L_FPT = 25
TILE = 16

# covering set: (nY, hidden, k, dtype, activation, scaler, thresholds, n)
CASES = [
    (1, (1,), 2, np.float32, "relu", None, False, 1),
    (3, (15,), 3, np.float64, "logistic", "meanstd", True, TILE - 1),
    (10, (16,), 11, np.float32, "tanh", "std", False, TILE),
    (16, (17,), 16, np.float64, "identity", None, True, TILE + 1),
    (17, (100,), 2, np.float32, "logistic", "meanstd", True, 100),
    (40, (512,), 11, np.float64, "relu", "std", False, 300),
    (40, (64, 32), 3, np.float32, "relu", "meanstd", True, 1000),
    (10, (100,), 11, np.float32, "logistic", None, True, 0),
    (17, (512,), 16, np.float32, "identity", "std", False, 33),
    (3, (64, 32), 2, np.float64, "tanh", None, False, 47),
    (40, (100, 50, 25, 12), 16, np.float32, "tanh", "std", True, 257),
    (16, (15,), 11, np.float32, "relu", None, True, 2000),
    (2601, (100,), 11, np.float32, "relu", None, True, 1000),
    (2601, (100, 50, 25, 12), 16, np.float64, "relu", "meanstd", False, 256),
    (2601, (17,), 3, np.float32, "logistic", "std", True, 129),
]


@functools.lru_cache(maxsize=None)
def _engine(nY):
    from warpdemux_amd.engine import DemuxEngine

    rng = np.random.default_rng(nY)
    refs = rng.normal(size=(nY, L_FPT))
    return DemuxEngine(refs, 15, 0.1, sig_proc.SegParams(barcode_num_events=L_FPT)), refs


def _distances(nY, n, seed):
    """(device float32 (n, nY) from the engine's DTW, host copy, the reads)"""
    import torch

    eng, refs = _engine(nY)
    rng = np.random.default_rng(seed)
    X = refs[rng.integers(0, nY, n)] + rng.normal(0, 0.7, size=(n, L_FPT)) if n else np.zeros((0, L_FPT))
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(eng.tdev)
    dist, _ = eng.dtw(Xd, want_argmin=False)
    return dist, dist.cpu().numpy(), X


def _wrap(est, refs, k, thresholds, seed):
    rng = np.random.default_rng(seed)
    lm = {i: int(v) for i, v in enumerate(rng.permutation(k) * 3 + 1)}
    thr = rng.uniform(0.05, 0.6, k) if thresholds else None
    return mlp_ref.DTW_MLP(est, refs, lm, thr, window=15, penalty=0.1, block_size=500)


def _run_tail(eng, dm, dist):
    import torch

    eng.set_mlp(dm)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.tdev)
    prob, pred, conf = eng.mlp_predict(dist, cnt)
    return prob.cpu().numpy(), pred.cpu().numpy(), conf.cpu().numpy(), int(cnt.item())


def _assert_contract(ref, est, D, prob, pred, conf, what):
    dtype = np.result_type(np.float32, mlp_ref.split_model(est)[1].coefs_[0].dtype)
    c = mlp_ref.contract(est, D, ref.thresholds)
    pred_sk, _ = mlp_ref.process_probs(c["p_sk"], ref.label_mapper, ref.thresholds)
    err, bad = mlp_ref.check_outputs(c, prob, conf, pred, pred_sk, dtype)
    ratio = err / c["e_ref"] if c["e_ref"] else float("nan")
    print(f"{what}: E_ref {c['e_ref']:.3g} T {c['T']:.3g} gpu err {err:.3g} (x{ratio:.3g} E_ref) "
          f"close {int(c['close'].sum())}/{len(D)}")
    assert c["close"].mean() <= 0.01 if len(D) else True, f"{what}: close-call cap"
    assert c["p_sk"].dtype == dtype
    assert not bad, f"{what}: {bad}"
    return c


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: "-".join(map(str, (CASES[i][0], "x".join(map(str, CASES[i][1])), CASES[i][2], np.dtype(CASES[i][3]).name, CASES[i][4], CASES[i][5] or "noscale", "thr" if CASES[i][6] else "nothr", CASES[i][7]))))
def test_tail_meets_the_contract(case):
    nY, hidden, k, dtype, act, sc, thr, n = CASES[case]
    eng, refs = _engine(nY)
    dist, D, _ = _distances(nY, n, seed=10 + case)
    fitD = D if n >= 2 else _distances(nY, 64, seed=99)[1]
    est = mlp_ref.with_scaler(mlp_ref.random_mlp(nY, hidden, k, dtype, act, seed=case), fitD, sc)
    ref = _wrap(est, refs, k, thr, seed=case)
    dm = models.from_reference(ref)
    assert isinstance(dm, models.DTW_MLP) and dm.dtype == dtype
    prob, pred, conf, cnt = _run_tail(eng, dm, dist)
    assert cnt == 0 and prob.shape == (n, k)
    if n == 0:   # (scikit-learn refuses an empty call; the device call enqueues nothing)
        return
    _assert_contract(ref, est, D, prob, pred, conf, f"case {case}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_trained_model(dtype):
    nY, k = 40, 4
    eng, refs = _engine(nY)
    rng = np.random.default_rng(5)
    cls = rng.integers(0, k, 800)
    centres = refs[:k]
    import torch

    X = centres[cls] + rng.normal(0, 0.8, size=(800, L_FPT))
    dist, _ = eng.dtw(torch.from_numpy(X).to(eng.tdev), want_argmin=False)
    D = dist.cpu().numpy()
    est = mlp_ref.with_scaler(mlp_ref.trained_mlp(D[:400], cls[:400], (20,), dtype, seed=1), D[:400], "meanstd")
    ref = _wrap(est, refs, k, True, seed=2)
    prob, pred, conf, cnt = _run_tail(eng, models.from_reference(ref), dist)
    assert cnt == 0
    _assert_contract(ref, est, D, prob, pred, conf, f"trained {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("act", ["relu", "identity"])
def test_exact_data(dtype, act):
    """Dyadic weights and integer distances: every summation order gives the same logits, so T is ulp-tight."""
    import torch

    nY, k, hidden = 40, 11, (17,)
    eng, refs = _engine(nY)
    rng = np.random.default_rng(11)
    D = rng.integers(0, 5, size=(200, nY)).astype(np.float32)
    est = mlp_ref.random_mlp(nY, hidden, k, dtype, act, seed=3)
    est.coefs_ = [(rng.integers(-4, 5, W.shape) / 64).astype(dtype) for W in est.coefs_]
    est.intercepts_ = [(rng.integers(-4, 5, b.shape) / 64).astype(dtype) for b in est.intercepts_]
    ref = _wrap(est, refs, k, True, seed=4)
    prob, pred, conf, cnt = _run_tail(eng, models.from_reference(ref), torch.from_numpy(D).to(eng.tdev))
    _assert_contract(ref, est, D, prob, pred, conf, f"exact {np.dtype(dtype).name} {act}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_positive_control(dtype):
    """A first-layer weight moved so that the exact outputs move by >= 10 T: the device result of the perturbed model fails
    the check against the unperturbed exact outputs."""
    nY, k = 40, 11
    eng, refs = _engine(nY)
    dist, D, _ = _distances(nY, 300, seed=7)
    est = mlp_ref.random_mlp(nY, (100,), k, dtype, "relu", seed=7)
    ref = _wrap(est, refs, k, False, seed=7)
    c = mlp_ref.contract(est, D, None)
    e2, moved = mlp_ref.perturb_first_layer(est, D, c["T"])
    prob, pred, conf, _ = _run_tail(eng, models.from_reference(_wrap(e2, refs, k, False, seed=7)), dist)
    pred_sk, _ = mlp_ref.process_probs(c["p_sk"], ref.label_mapper, None)
    err, bad = mlp_ref.check_outputs(c, prob, conf, pred, pred_sk, dtype)
    print(f"positive control {np.dtype(dtype).name}: moved {moved:.3g}, T {c['T']:.3g}, gpu err {err:.3g}")
    assert moved >= 10 * c["T"] and bad
    # the unperturbed model passes on the same distances
    prob, pred, conf, _ = _run_tail(eng, models.from_reference(ref), dist)
    assert not mlp_ref.check_outputs(c, prob, conf, pred, pred_sk, dtype)[1]


def _synth_reads(n, seed):
    """(device sig, offsets, a_start, a_end, ok) of n synthetic reads, a few with detect failure"""
    import torch

    spec = synth.SynthSpec(n_barcodes=4, seed=seed)
    mb, a_s, a_e, _ = synth.generate_minibatch(spec, 0, n, 8000)
    ok = np.ones(n, dtype=np.uint8)
    ok[::9] = 0
    dev = "cuda"
    return (torch.from_numpy(mb).to(dev), torch.from_numpy(a_s.astype(np.int32)).to(dev),
            torch.from_numpy(a_e.astype(np.int32)).to(dev), torch.from_numpy(ok).to(dev), mb.shape[1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_entry_points_agree_bitwise(dtype):
    """wdx_demux_mlp_dev (small row blocks) = wdx_mlp_predict_dev on its distances = wdx_dtw_mlp_predict over >= 3 row
    chunks = DTW_MLP.predict, bit for bit; reads whose fingerprint failed get -1 / NaN and are not counted."""
    import torch

    from warpdemux_amd.engine import DemuxEngine

    n = 150
    sig, a_s, a_e, ok, stride = _synth_reads(n, seed=3)
    probe = DemuxEngine(np.zeros((1, L_FPT)), 15, 0.1, sig_proc.SegParams(barcode_num_events=L_FPT))
    fpt, _, _, st = probe.fingerprint(sig, a_s, a_e, stride=stride, max_len=stride, ok=ok)
    good = (st == 0).cpu().numpy()
    refs = fpt.cpu().numpy()[good][:40] + 0.01
    probe.close()
    eng = DemuxEngine(refs, 15, 0.1, sig_proc.SegParams(barcode_num_events=L_FPT))
    D0 = eng.dtw(fpt[torch.from_numpy(good).to(fpt.device)], want_argmin=False)[0].cpu().numpy()
    est = mlp_ref.with_scaler(mlp_ref.random_mlp(len(refs), (64, 32), 11, dtype, "relu", seed=9), D0, "meanstd")
    ref = _wrap(est, refs, 11, True, seed=9)
    dm = models.from_reference(ref)
    eng.set_mlp(dm)
    cnt = torch.zeros(1, dtype=torch.int64, device=eng.tdev)
    prob, pred, conf, status, dist, fptd = (t.cpu().numpy() if t is not None else None for t in eng.demux_mlp(
        sig, a_s, a_e, stride=stride, max_len=stride, ok=ok, want_dist=True, want_fpt=True, block_rows=37, n_nonfinite=cnt))
    good = status == 0
    assert 0 < good.sum() < n and cnt.item() == 0
    assert (pred[~good] == -1).all() and np.isnan(prob[~good]).all() and np.isnan(conf[~good]).all()
    # the tail alone on the same distances
    p2, pr2, c2 = (t.cpu().numpy() for t in eng.mlp_predict(torch.from_numpy(dist[good]).to(eng.tdev)))
    assert np.array_equal(p2, prob[good]) and np.array_equal(pr2, pred[good]) and np.array_equal(c2, conf[good])
    # host-buffer form over several row chunks
    X = np.ascontiguousarray(fptd[good])
    m = len(X)
    eng.ctx.set_option(_lib.OPT_MLP_CHUNK_ROWS, (m + 2) // 3 - 1)
    try:
        p3, pr3, c3 = np.empty((m, 11)), np.empty(m, np.int32), np.empty(m)
        bad = C.c_int64(-1)
        _lib.check(_lib.load().wdx_dtw_mlp_predict(eng.ctx.handle, _lib.ptr(X), m, _lib.ptr(p3), _lib.ptr(pr3), _lib.ptr(c3),
                                                   C.byref(bad)))
    finally:
        eng.ctx.set_option(_lib.OPT_MLP_CHUNK_ROWS, 0)
    assert bad.value == 0
    assert np.array_equal(p3, prob[good]) and np.array_equal(pr3, pred[good]) and np.array_equal(c3, conf[good])
    # the Python model
    y_pred, y_prob = dm.predict(X)
    assert y_prob.dtype == dtype
    assert np.array_equal(y_prob.astype(np.float64), prob[good]) and np.array_equal(y_pred, pred[good].astype(np.int64))
    _assert_contract(ref, est, dist[good], prob[good], pred[good], conf[good], "demux")


def test_nonfinite_rows_are_masked_counted_and_raise():
    import torch

    nY, k = 17, 5
    eng, refs = _engine(nY)
    dist, D, X = _distances(nY, 40, seed=21)
    est = mlp_ref.random_mlp(nY, (16,), k, np.float32, "relu", seed=21)
    ref = _wrap(est, refs, k, False, seed=21)
    prob0, pred0, conf0, _ = _run_tail(eng, models.from_reference(ref), dist)
    Db = D.copy()
    Db[3, 0], Db[17, 16], Db[18, 5], Db[30, :] = np.nan, np.inf, -np.inf, np.nan
    prob, pred, conf, cnt = _run_tail(eng, models.from_reference(ref), torch.from_numpy(Db).to(eng.tdev))
    rows = [3, 17, 18, 30]
    other = np.setdiff1d(np.arange(40), rows)
    assert cnt == 4
    assert (pred[rows] == -1).all() and np.isnan(prob[rows]).all() and np.isnan(conf[rows]).all()
    assert np.array_equal(prob[other], prob0[other]) and np.array_equal(pred[other], pred0[other])
    # DTW_MLP.predict refuses the call with scikit-learn's first line
    Xb = X.copy()
    Xb[2, 4] = np.nan
    with pytest.raises(ValueError) as sk:
        est.predict_proba(np.where(np.arange(40)[:, None] == 2, np.nan, D).astype(np.float32))
    with pytest.raises(ValueError) as got:
        models.from_reference(ref).predict(Xb)
    assert str(got.value).splitlines()[0] == str(sk.value).splitlines()[0]


def _model_c(nY, hidden, k, dtype=np.float32, n_out=None, n_scalers=0):
    rng = np.random.default_rng(0)
    sizes = [nY, *hidden, k if n_out is None else n_out]
    keep = [rng.normal(size=(a, b)).astype(dtype) for a, b in zip(sizes[:-1], sizes[1:])]
    keep += [rng.normal(size=b).astype(dtype) for b in sizes[1:]]
    sc = [np.ones(nY) for _ in range(n_scalers)]
    m = _lib.MlpModelC()
    m.n_layers, m.dtype_bytes, m.hidden_activation, m.n_classes, m.n_scalers = len(sizes) - 1, np.dtype(dtype).itemsize, 3, k, n_scalers
    if len(sizes) <= _lib.MLP_MAX_LAYERS + 1:
        for i, s in enumerate(sizes):
            m.sizes[i] = s
        for i in range(len(sizes) - 1):
            m.coefs[i] = keep[i].ctypes.data
            m.intercepts[i] = keep[len(sizes) - 1 + i].ctypes.data
    for i in range(min(n_scalers, _lib.MLP_MAX_SCALERS)):
        m.scaler_scale[i] = sc[i].ctypes.data
    return m, (keep, sc)


def test_limits_refusals_and_no_model():
    from warpdemux_amd.engine import DemuxEngine

    nY = 10
    eng, refs = _engine(nY)
    L = _lib.load()
    # no model yet on a fresh context
    fresh = DemuxEngine(refs, 15, 0.1, sig_proc.SegParams(barcode_num_events=L_FPT))
    dist, D, X = _distances(nY, 20, seed=1)
    assert L.wdx_mlp_predict_dev(fresh.ctx.handle, C.c_void_p(dist.data_ptr()), 20, None, None, None, None, None) == _lib.WDX_ERR_NO_REFS
    assert L.wdx_dtw_mlp_predict(fresh.ctx.handle, _lib.ptr(X), 20, None, None, None, None) == _lib.WDX_ERR_NO_REFS
    fresh.close()
    est = mlp_ref.random_mlp(nY, (16,), 4, np.float32, "relu", seed=1)
    ref = _wrap(est, refs, 4, True, seed=1)
    prob0, pred0, conf0, _ = _run_tail(eng, models.from_reference(ref), dist)

    def rc(**kw):
        m, keep = _model_c(nY, **kw)
        return L.wdx_mlp_set_model(eng.ctx.handle, C.byref(m))

    ok, unsup, inval = _lib.WDX_SUCCESS, _lib.WDX_ERR_UNSUPPORTED, _lib.WDX_ERR_INVALID
    cases = [
        (dict(hidden=(16,), k=16), ok), (dict(hidden=(16,), k=17), unsup), (dict(hidden=(16,), k=1), inval),
        (dict(hidden=(512,), k=3), ok), (dict(hidden=(513,), k=3), unsup), (dict(hidden=(0,), k=3), inval),
        (dict(hidden=(4, 4, 4, 4), k=3), ok), (dict(hidden=(4, 4, 4, 4, 4), k=3), unsup), (dict(hidden=(), k=3), unsup),
        (dict(hidden=(8,), k=2, n_out=1), ok), (dict(hidden=(8,), k=3, n_out=1), inval), (dict(hidden=(8,), k=3, n_out=4), inval),
        (dict(hidden=(8,), k=3, n_scalers=4), ok), (dict(hidden=(8,), k=3, n_scalers=5), unsup),
    ]
    for kw, want in cases:
        got = rc(**kw)
        print(kw, got, want)
        assert got == want, (kw, got, want)
    m, keep = _model_c(nY, (8,), 3)
    m.dtype_bytes = 2
    assert L.wdx_mlp_set_model(eng.ctx.handle, C.byref(m)) == inval
    m, keep = _model_c(nY, (8,), 3)
    m.coefs[1] = None
    assert L.wdx_mlp_set_model(eng.ctx.handle, C.byref(m)) == inval
    # a refused model keeps the previous one
    dm = models.from_reference(ref)
    eng.set_mlp(dm)
    assert rc(hidden=(513,), k=3) == unsup and rc(hidden=(8,), k=3, n_out=4) == inval
    prob, pred, conf = (t.cpu().numpy() for t in eng.mlp_predict(dist))
    assert np.array_equal(prob, prob0) and np.array_equal(pred, pred0) and np.array_equal(conf, conf0)
    # len(_X) != n_in
    m, keep = _model_c(nY + 1, (8,), 3)
    assert L.wdx_mlp_set_model(eng.ctx.handle, C.byref(m)) == ok
    assert L.wdx_dtw_mlp_predict(eng.ctx.handle, _lib.ptr(X), 20, None, None, None, None) == inval
    # Python limits surface as NotImplementedError, malformed pipelines as ValueError
    with pytest.raises(NotImplementedError):
        big = mlp_ref.random_mlp(nY, (600,), 3, np.float32, "relu", seed=2)
        eng.set_mlp(models.from_reference(_wrap(big, refs, 3, False, seed=2)))
    from sklearn.decomposition import PCA
    from sklearn.pipeline import Pipeline

    with pytest.raises(ValueError):
        models.from_reference(_wrap(Pipeline([("pca", PCA(2).fit(D)), ("mlp", est)]), refs, 4, False, seed=1))
    with pytest.raises(ValueError, match="axis 1"):
        models.from_reference(ref).predict(np.zeros((2, L_FPT + 1)))
    with pytest.raises(ValueError, match="block_size"):
        dm2 = models.from_reference(ref)
        dm2.block_size = None
        dm2.predict(X, nproc=-1)
    assert models.from_reference(ref).num_bcs() == 4     # len(label_mapper) - noise_class


def test_svm_unaffected_by_an_mlp():
    """DTW_SVM.predict is bitwise the same before and after an MLP is set on the same context and references."""
    k = 5
    sm = svm_ref.synth_model(k, seed=3)
    rng = np.random.default_rng(3)
    refs = rng.normal(size=(sm.n_train, L_FPT))
    svm = models.DTW_SVM(refs, sm.n_support, sm.support, sm.dual_coef, sm.rho, sm.probA, sm.probB,
                         {i: int(v) for i, v in enumerate(sm.label_map)}, sm.thresholds, 15, 0.1, block_size=500)
    X = refs[rng.integers(0, sm.n_train, 200)] + rng.normal(0, 0.5, size=(200, L_FPT))
    a_pred, a_prob = svm.predict(X)
    est = mlp_ref.random_mlp(sm.n_train, (32,), 7, np.float32, "relu", seed=3)
    mlp = models.from_reference(_wrap(est, refs, 7, True, seed=3))
    mlp.predict(X)
    b_pred, b_prob = svm.predict(X)
    assert np.array_equal(a_pred, b_pred) and np.array_equal(a_prob, b_prob)
