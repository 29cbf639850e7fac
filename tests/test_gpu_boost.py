"""The Fpt_Boost classifier tail on the device (wdx_boost.hip) against its NumPy restatement
(tests/helpers/boost_ref.py): raw scores bit for bit, probabilities under the accuracy contract T = 4 max(E_ref, 2**-53),
the tail, the model slot, the chunked host call and the tRNA flow in one call.  CatBoost itself is compared only where it
can be imported (the last test).  Every case prints its figures before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import boost_ref, mlp_ref, svm_ref
from helpers import refine_inputs as ri
from warpdemux_amd import _lib, models, sig_proc

pytestmark = pytest.mark.gpu

K_FPT = 25
NS = (1, 63, 64, 65, 1000)      # one read, a partial wave, a full wave, one read into the second wave, 16 waves
MIXED = (0, 1, 6, 10, 3)

# the bit-for-bit shapes: the whole product trees x depth x dim x features, each at every n of NS
TREES, DEPTHS, DIMS, FEATURES = (1, 3, 257), (0, 1, 6, 10, MIXED), (1, 4, 16), (1, 25, 64)
# ... and the class counts on both sides of every bound of the kernel's dispatch (DMAX 1 | 4 | 8 | 16): 2 and 3 with 4 under
# <4>, 5 and 8 under <8>, 9 under <16>
DISPATCH = [(3, 6, 2, 25), (257, 1, 3, 64), (3, 6, 5, 25), (257, MIXED, 5, 64), (257, 10, 8, 25), (1, 0, 8, 1), (3, MIXED, 9, 25)]
# (n_trees, depth, dim, n_features); thresholds on in every second case, the NaN treatment cycles through the three
CASES = [(t, d, dim, f) for t in TREES for d in DEPTHS for dim in DIMS for f in FEATURES] + DISPATCH
assert len(CASES) == 135 + len(DISPATCH)


@functools.lru_cache(maxsize=None)
def _engine():
    from warpdemux_amd.engine import DemuxEngine

    return DemuxEngine(np.zeros((1, K_FPT)), 15, 0.1, sig_proc.SegParams(barcode_num_events=K_FPT, **ri.SEG))


def _labels(k, seed):
    rng = np.random.default_rng(seed)
    return {i: int(v) for i, v in enumerate(rng.permutation(k) * 3 + 1)}


def _device_model(m, label_mapper, thresholds=None):
    """models.Fpt_Boost straight from a restatement model (the JSON route is walked by the smaller tests)."""
    trees = [(f, b, [m.nan_treatment[i] == "AsTrue" for i in f], lv) for f, b, lv in m.trees]
    return models.Fpt_Boost(trees, m.n_features, m.scale, m.bias, label_mapper, thresholds)


def _run(eng, dm, X, status=None):
    import torch

    eng.set_boost(dm)
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(eng.tdev)
    sd = None if status is None else torch.from_numpy(np.asarray(status, dtype=np.int32)).to(eng.tdev)
    prob, pred, conf, raw = eng.boost_predict(Xd, sd, want_raw=True)
    return raw.cpu().numpy(), prob.cpu().numpy(), pred.cpu().numpy(), conf.cpu().numpy()


def _assert_contract(c, lm, thr, prob, pred, conf, what):
    pred_ref, _ = boost_ref.process_probs(c["p64"], lm, thr)
    err, bad = boost_ref.check_outputs(c, prob, conf, pred, pred_ref)
    ratio = err / c["e_ref"] if c["e_ref"] else float("nan")
    print(f"{what}: E_ref {c['e_ref']:.3g} T {c['T']:.3g} gpu err {err:.3g} (x{ratio:.3g} E_ref) "
          f"close {int(c['close'].sum())}/{len(prob)}")
    assert c["close"].mean() <= 0.01, f"{what}: close-call cap"
    assert not bad, f"{what}: {bad}"


def _case_id(i):
    t, d, dim, f = CASES[i]
    return f"{t}t-d{'mixed' if isinstance(d, tuple) else d}-dim{dim}-f{f}"


def _case(case):
    """The model, the rows, the label map and the thresholds of CASES[case] (also what the CPU check of the close-call cap
    walks: every case has no close call in the restatement alone)."""
    n_trees, depth, dim, n_features = CASES[case]
    nan = boost_ref.NAN_TREATMENTS[case % 3]
    m = boost_ref.random_model(n_trees, depth, dim, n_features, seed=100 + case, nan_treatment=[nan] * n_features)
    X = boost_ref.random_inputs(m, max(NS), seed=200 + case)
    X[5::97, 0] = np.nan                                     # a few NaN features in every case
    thr = np.random.default_rng(case).uniform(0.05, 0.6, m.k) if case % 2 else None
    return m, X, _labels(m.k, case), thr


@pytest.mark.parametrize("case", range(len(CASES)), ids=_case_id)
def test_raw_scores_bit_for_bit_and_probabilities_in_contract(case):
    m, X, lm, thr = _case(case)
    dim, k = m.dim, m.k
    dm = _device_model(m, lm, thr)
    eng = _engine()
    c = boost_ref.contract(m, X, thr)
    full = _run(eng, dm, X)
    for n in NS:
        raw, prob, pred, conf = full if n == max(NS) else _run(eng, dm, X[:n])
        assert raw.shape == (n, dim) and prob.shape == (n, k)
        same = np.array_equal(raw, c["raw"][:n])
        print(f"case {case} n {n}: raw bit for bit {same}")
        assert same, f"case {case} n {n}: max |raw - restatement| = {np.abs(raw - c['raw'][:n]).max():.3g}"
        # the rows of a shorter call are the first rows of the longest, bit for bit
        assert np.array_equal(prob, full[1][:n]) and np.array_equal(pred, full[2][:n]) and np.array_equal(conf, full[3][:n])
    _assert_contract(c, lm, thr, *full[1:], f"case {case}")


def test_borders_nan_and_infinities():
    """x == border is false; a float64 above the border that rounds to it in float32 is false; the next float32 is true;
    NaN follows each of the three treatments; +inf is true and -inf false.  Expected leaves are written out, not computed."""
    b = np.float32(0.1)
    up32 = np.nextafter(b, np.float32(np.inf))
    above_rounds_down = float(b) * (1 + 2.0 ** -30)
    assert np.float32(above_rounds_down) == b and above_rounds_down > float(b)
    # three features (AsIs, AsFalse, AsTrue), one depth-1 tree each; the "greater" leaf of feature j is worth 2**j
    trees = [([j], [b], [[0.0], [2.0 ** j]]) for j in range(3)]
    m = boost_ref.BoostModel(trees, 3, 1, 1.0, [0.0], nan_treatment=["AsIs", "AsFalse", "AsTrue"])
    rows = [
        ([float(b)] * 3, 0.0),
        ([above_rounds_down] * 3, 0.0),
        ([float(up32)] * 3, 7.0),
        ([np.nan] * 3, 4.0),                                  # only AsTrue sets its bit
        ([np.inf] * 3, 7.0),
        ([-np.inf] * 3, 0.0),
        ([np.nan, 1.0, -1.0], 2.0),
        ([1.0, np.nan, np.nan], 5.0),
    ]
    X = np.array([r for r, _ in rows])
    want = np.array([[w] for _, w in rows])
    assert np.array_equal(boost_ref.raw_scores(m, X), want)
    raw, prob, pred, conf = _run(_engine(), _device_model(m, {0: 0, 1: 1}), X)
    print("borders raw", raw.ravel())
    assert np.array_equal(raw, want)
    # the same through the JSON loader
    raw2 = _run(_engine(), models.Fpt_Boost.from_json(boost_ref.to_json(m), {0: 0, 1: 1}), X)[0]
    assert np.array_equal(raw2, want)


def test_negative_control():
    """One leaf value moved until the exact outputs move by >= 10 T: the device result of the perturbed model fails the check
    against the unperturbed exact outputs; the unperturbed model passes on the same rows."""
    m = boost_ref.random_model(257, 6, 4, K_FPT, seed=31)
    X = boost_ref.random_inputs(m, 300, seed=32)
    lm = _labels(4, 3)
    c = boost_ref.contract(m, X)
    m2, moved = boost_ref.perturb_leaf(m, X, c["T"])
    pred_ref, _ = boost_ref.process_probs(c["p64"], lm)
    raw, prob, pred, conf = _run(_engine(), _device_model(m2, lm), X)
    err, bad = boost_ref.check_outputs(c, prob, conf, pred, pred_ref)
    print(f"negative control: moved {moved:.3g}, T {c['T']:.3g}, gpu err {err:.3g}")
    assert moved >= 10 * c["T"] and bad and not np.array_equal(raw, c["raw"])
    raw, prob, pred, conf = _run(_engine(), _device_model(m, lm), X)
    assert np.array_equal(raw, c["raw"]) and not boost_ref.check_outputs(c, prob, conf, pred, pred_ref)[1]


def test_tail_label_map_thresholds_tie_and_sigmoid():
    eng = _engine()
    # an exact tie between classes 1 and 2 (equal leaves, equal bias): first maximum, margin 0
    lv = np.array([[0.0, 2.0, 2.0, -1.0], [0.5, 3.0, 3.0, 0.0]])
    m = boost_ref.BoostModel([([0], [0.0], lv)], 1, 4, 1.5, [0.25, 0.5, 0.5, 0.0])
    X = np.array([[-1.0], [1.0]])
    lm = {0: 10, 1: 20, 2: 30, 3: 40}
    raw, prob, pred, conf = _run(eng, _device_model(m, lm), X)
    assert np.array_equal(raw, boost_ref.raw_scores(m, X)) and (prob[:, 1] == prob[:, 2]).all()
    assert pred.tolist() == [20, 20] and conf.tolist() == [0.0, 0.0]
    # ... and any positive threshold of the winning class rejects it; the other classes' thresholds do not matter
    assert _run(eng, _device_model(m, lm, np.array([0.0, 1e-300, 9.0, 9.0])), X)[2].tolist() == [-1, -1]
    assert _run(eng, _device_model(m, lm, np.array([9.0, 0.0, 9.0, 9.0])), X)[2].tolist() == [20, 20]
    # k = 2 through the sigmoid: raw 0 -> [0.5, 0.5], the first class wins; raw > 0 -> class 1
    m1 = boost_ref.BoostModel([([0], [0.0], [[0.0], [2.0]])], 1, 1, 1.0, [0.0])
    raw, prob, pred, conf = _run(eng, _device_model(m1, {0: 5, 1: 6}), X)
    assert raw.ravel().tolist() == [0.0, 2.0] and prob[0].tolist() == [0.5, 0.5] and pred.tolist() == [5, 6]
    p1 = 1 / (1 + np.exp(-2.0))
    assert abs(prob[1, 1] - p1) <= 4 * 2.0 ** -53 and prob[1, 0] == 1 - prob[1, 1] and conf[1] == prob[1, 1] - prob[1, 0]
    # thresholds on and off on a random model: the same probabilities, -1 exactly where the margin is below the threshold
    m = boost_ref.random_model(3, 6, 4, K_FPT, seed=41)
    X = boost_ref.random_inputs(m, 500, seed=42)
    lm = _labels(4, 9)
    thr = np.array([0.2, 0.5, 0.1, 0.8])
    raw0, prob0, pred0, conf0 = _run(eng, _device_model(m, lm), X)
    raw1, prob1, pred1, conf1 = _run(eng, _device_model(m, lm, thr), X)
    assert np.array_equal(prob0, prob1) and np.array_equal(conf0, conf1) and set(pred0) <= set(lm.values())
    cut = conf1 < thr[np.argmax(prob1, axis=1)]
    assert 0 < cut.sum() < len(X) and (pred1[cut] == -1).all() and np.array_equal(pred1[~cut], pred0[~cut])
    # failed reads (status != 0): -1 and NaN, the others untouched
    st = np.zeros(len(X), dtype=np.int32)
    st[[0, 63, 64, 499]] = (1, 3, 6, 2)
    raw2, prob2, pred2, conf2 = _run(eng, _device_model(m, lm, thr), X, st)
    f = st != 0
    assert (pred2[f] == -1).all() and np.isnan(prob2[f]).all() and np.isnan(conf2[f]).all() and np.isnan(raw2[f]).all()
    assert np.array_equal(prob2[~f], prob1[~f]) and np.array_equal(pred2[~f], pred1[~f]) and np.array_equal(raw2[~f], raw1[~f])


def _model_c(n_features=4, dim=3, k=None, depth=(2, 1), feature=0):
    k = (2 if dim == 1 else dim) if k is None else k
    depth_a = np.array(depth, dtype=np.int32)
    ns = int(np.maximum(depth_a, 0).sum())   # (a negative depth is one of the refusals: it owns no splits)
    keep = [depth_a, np.full(ns, feature, dtype=np.int32), np.zeros(ns, dtype=np.float32), np.zeros(ns, dtype=np.uint8),
            np.ones(int(sum(1 << max(d, 0) for d in depth)) * max(dim, 1), dtype=np.float64), np.zeros(max(dim, 1))]
    m = _lib.BoostModelC(len(depth), n_features, dim, k, *(a.ctypes.data for a in keep[:5]), 1.0, keep[5].ctypes.data, None, None)
    return m, keep


def test_model_slot_limits_and_refusals():
    from warpdemux_amd.engine import DemuxEngine

    eng = _engine()
    L = _lib.load()
    ok, unsup, inval = _lib.WDX_SUCCESS, _lib.WDX_ERR_UNSUPPORTED, _lib.WDX_ERR_INVALID
    fresh = DemuxEngine(np.zeros((1, K_FPT)), 15, 0.1, sig_proc.SegParams(barcode_num_events=K_FPT))
    X = np.zeros((4, K_FPT))
    assert L.wdx_boost_predict(fresh.ctx.handle, _lib.ptr(X), 4, None, None, None, None) == _lib.WDX_ERR_NO_REFS
    assert L.wdx_boost_predict_dev(fresh.ctx.handle, None, None, 0, None, None, None, None, None) == _lib.WDX_ERR_NO_REFS
    fresh.close()
    m = boost_ref.random_model(3, 6, 4, K_FPT, seed=51)
    Xr = boost_ref.random_inputs(m, 200, seed=52)
    lm = _labels(4, 5)
    base = _run(eng, _device_model(m, lm), Xr)

    def rc(**kw):
        mc, keep = _model_c(**kw)
        return L.wdx_boost_set_model(eng.ctx.handle, C.byref(mc))

    refused = [
        (dict(dim=17), unsup), (dict(depth=(17,), dim=1), unsup), (dict(n_features=255), unsup),
        (dict(dim=3, k=4), inval), (dict(dim=1, k=3), inval), (dict(n_features=0), inval), (dict(depth=(-1,)), inval),
        (dict(feature=4), inval), (dict(feature=-1), inval), (dict(depth=()), inval), (dict(dim=0), inval),
    ]
    for kw, want in refused:
        got = rc(**kw)
        print(kw, got, want)
        assert got == want, (kw, got, want)
        assert _lib.load().wdx_last_error()
    # a refused model keeps the previous one
    import torch

    Xd = torch.from_numpy(Xr).to(eng.tdev)
    prob, pred, conf, raw = (t.cpu().numpy() for t in eng.boost_predict(Xd, want_raw=True))
    assert np.array_equal(raw, base[0]) and np.array_equal(prob, base[1]) and np.array_equal(pred, base[2])
    # the limits themselves are accepted, and replacing the model mid-stream gives the new answers
    for kw in (dict(dim=16), dict(depth=(16,), dim=1), dict(n_features=254, feature=253), dict(depth=(0,), dim=1)):
        assert rc(**kw) == ok, kw
    # the widest row the fingerprint stage can write: 254 features (more than 64 KB of LDS per wave), depth 16
    mw = boost_ref.random_model(2, [16, 3], 2, 254, seed=54)
    Xw = boost_ref.random_inputs(mw, 65, seed=55)
    assert np.array_equal(_run(eng, _device_model(mw, {0: 1, 1: 0}), Xw)[0], boost_ref.raw_scores(mw, Xw))
    m2 = boost_ref.random_model(5, MIXED, 4, K_FPT, seed=53)
    eng.set_boost(_device_model(m, lm))
    eng.boost_predict(Xd)                                      # (a launch of the old model is in flight or done)
    got = _run(eng, _device_model(m2, lm), Xr)
    assert np.array_equal(got[0], boost_ref.raw_scores(m2, Xr)) and not np.array_equal(got[0], base[0])
    # Python-side limits surface as NotImplementedError before the library is asked
    with pytest.raises(NotImplementedError):
        _device_model(boost_ref.random_model(1, 1, 17, 3, seed=1), {i: i for i in range(17)})
    # feature count != fingerprint length in the fused call
    eng.set_boost(_device_model(boost_ref.random_model(1, 1, 4, K_FPT + 1, seed=1), lm))
    b = ri.batch(3)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.tdev)   # noqa: E731
    with pytest.raises(ValueError, match="features"):
        eng.demux_boost(d(b["rows"]), d(b["a_s"]), d(b["a_e"]), max_len=b["rows"].shape[1], ok=d(b["ok"]))


def test_svm_and_mlp_unaffected_by_a_boost_model():
    """DTW_SVM.predict and DTW_MLP.predict are bitwise the same before and after a boost model is set on the same context."""
    k = 5
    sm = svm_ref.synth_model(k, seed=3)
    rng = np.random.default_rng(3)
    refs = rng.normal(size=(sm.n_train, K_FPT))
    svm = models.DTW_SVM(refs, sm.n_support, sm.support, sm.dual_coef, sm.rho, sm.probA, sm.probB,
                         {i: int(v) for i, v in enumerate(sm.label_map)}, sm.thresholds, 15, 0.1, block_size=500)
    est = mlp_ref.random_mlp(sm.n_train, (32,), 7, np.float32, "relu", seed=3)
    mlp = models.from_reference(mlp_ref.DTW_MLP(est, refs, _labels(7, 1), None, window=15, penalty=0.1, block_size=500))
    X = refs[rng.integers(0, sm.n_train, 200)] + rng.normal(0, 0.5, size=(200, K_FPT))
    a = svm.predict(X), mlp.predict(X)
    m = boost_ref.random_model(3, 6, 4, K_FPT, seed=61)
    fb = models.from_reference(boost_ref.Fpt_Boost(m, _labels(4, 2)))
    y_pred, conf = fb.predict(X)
    c = boost_ref.contract(m, X)
    assert np.array_equal(fb.predict_raw(X)[0], c["raw"]) and y_pred.dtype == np.int64 and conf.shape == (200,)
    b = svm.predict(X), mlp.predict(X)
    for u, v in zip(a, b):
        assert np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1])
    # ... and the boost model is still resident and the same
    assert np.array_equal(fb.predict(X)[0], y_pred)


def test_host_call_in_chunks_and_python_predict():
    m = boost_ref.random_model(257, MIXED, 4, K_FPT, seed=71)
    X = boost_ref.random_inputs(m, 1000, seed=72)
    lm = _labels(4, 7)
    thr = np.array([0.1, 0.3, 0.2, 0.4])
    fb = models.from_reference(boost_ref.Fpt_Boost(m, lm, thr))      # the JSON route on a 257-tree model
    raw, prob, pred, conf = fb.predict_raw(X)
    c = boost_ref.contract(m, X, thr)
    assert np.array_equal(raw, c["raw"])
    _assert_contract(c, lm, thr, prob, pred, conf, "host call")
    ctx = _lib.default_context()
    ctx.set_option(_lib.OPT_BOOST_CHUNK_ROWS, 333)                   # 333 + 333 + 333 + 1 rows
    try:
        raw2, prob2, pred2, conf2 = fb.predict_raw(X)
        ctx.set_option(_lib.OPT_BOOST_CHUNK_ROWS, 64)
        raw3 = fb.predict_raw(X)[0]
    finally:
        ctx.set_option(_lib.OPT_BOOST_CHUNK_ROWS, 0)
    assert np.array_equal(raw2, raw) and np.array_equal(prob2, prob) and np.array_equal(pred2, pred) and np.array_equal(conf2, conf)
    assert np.array_equal(raw3, raw)
    # the reference's return values: (y_pred, conf), or the DataFrame; extra arguments are ignored; a 1-D X is one row
    y_pred, y_conf = fb.predict(X, nproc=4, pbar=True)
    assert np.array_equal(y_pred, pred) and np.array_equal(y_conf, conf)
    y1, c1 = fb.predict(X[7])
    assert y1.shape == (1,) and y1[0] == pred[7] and c1[0] == conf[7]
    df = fb.predict(X[:20], return_df=True)
    assert list(df.columns) == ["predicted_barcode", "confidence_score"] + [f"p{lm[i]:02d}" for i in range(4)]
    assert np.array_equal(df["predicted_barcode"].to_numpy(), pred[:20])
    assert np.array_equal(df["confidence_score"].to_numpy(), conf[:20].round(3))


@pytest.mark.parametrize("refine", [True, False], ids=["refine", "plain"])
def test_trna_flow_in_one_call(refine):
    """wdx_demux_boost_dev = fingerprint_refine_batch (or fingerprint_batch) followed by Fpt_Boost.predict on the successful
    rows: fpt / status / refine_idx / raw bit for bit, prob / pred / conf identical; failed reads carry -1 / NaN."""
    import torch

    eng = _engine()
    b = ri.batch(11, n=300)
    hp = sig_proc.SegParams(barcode_num_events=K_FPT, **ri.SEG)
    hr = sig_proc.RefineParams(query=ri.consensus(), **ri.REF)
    fbatch = (sig_proc.fingerprint_refine_batch(b["rows"], b["a_s"], b["a_e"], hp, hr, success=b["ok"]) if refine
              else sig_proc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], hp, success=b["ok"]))
    good = fbatch.status == 0
    if refine:
        ri.check_kinds(fbatch.status, False)
    assert 40 <= good.sum() < 300 and fbatch.status[ri.I_DEAD] == 1 and fbatch.status[ri.I_SHORT] == 3
    m = boost_ref.random_model(257, 6, 4, K_FPT, seed=81)
    # fingerprints are normalised event means: the model's borders (U(-1.5, 1.5)) cut through them
    lm = _labels(4, 8)
    thr = np.array([0.05, 0.2, 0.1, 0.3])
    dm = _device_model(m, lm, thr)
    eng.set_boost(dm)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.tdev)   # noqa: E731
    stride = b["rows"].shape[1]
    prob, pred, conf, status, idx, fpt, raw = (t.cpu().numpy() if t is not None else None for t in eng.demux_boost(
        d(b["rows"]), d(b["a_s"]), d(b["a_e"]), hr if refine else None, stride=stride, max_len=stride, ok=d(b["ok"]),
        want_fpt=True, want_raw=True))
    assert np.array_equal(status, fbatch.status)
    assert np.array_equal(fpt, fbatch.fpt, equal_nan=True)
    if refine:
        assert np.array_equal(idx, fbatch.refine_idx) and (status == 6).sum() >= 3
    else:
        assert idx is None
    raw_h, prob_h, pred_h, conf_h = dm.predict_raw(fbatch.fpt[good])
    c = boost_ref.contract(m, fbatch.fpt[good], thr)
    assert np.array_equal(raw_h, c["raw"]) and np.array_equal(raw[good], c["raw"])
    assert np.array_equal(prob[good], prob_h) and np.array_equal(pred[good], pred_h) and np.array_equal(conf[good], conf_h)
    leaves_hit = len({tuple(r) for r in boost_ref.leaf_indices(m, fbatch.fpt[good])[:8].T})
    print(f"tRNA flow ({'refine' if refine else 'plain'}): {int(good.sum())} good reads, {leaves_hit} distinct leaf tuples")
    assert leaves_hit > 10                                     # the fingerprints do walk different leaves
    _assert_contract(c, lm, thr, prob[good], pred[good], conf[good], "tRNA flow")
    bad = ~good
    assert (pred[bad] == -1).all() and np.isnan(prob[bad]).all() and np.isnan(conf[bad]).all() and np.isnan(raw[bad]).all()
    # without the optional outputs the required ones are the same
    p2, pr2, c2, st2, _, f2, r2 = eng.demux_boost(d(b["rows"]), d(b["a_s"]), d(b["a_e"]), hr if refine else None, stride=stride,
                                                  max_len=stride, ok=d(b["ok"]))
    assert f2 is None and r2 is None and np.array_equal(pr2.cpu().numpy(), pred) and np.array_equal(st2.cpu().numpy(), status)
    assert np.array_equal(p2.cpu().numpy(), prob, equal_nan=True)


@pytest.mark.parametrize("loss", ["MultiClass", "Logloss"])
def test_catboost_cross_check_if_available(loss, tmp_path):
    """Pins the restatement and the device to CatBoost itself wherever the library can be imported (nowhere this project is
    built today): RawFormulaVal against the raw scores, predict_proba against the probabilities."""
    cb = pytest.importorskip("catboost")
    rng = np.random.default_rng(0)
    k = 4 if loss == "MultiClass" else 2
    Xt = rng.normal(size=(400, K_FPT))
    yt = (Xt[:, :k].argmax(axis=1) + (rng.random(400) < 0.1)) % k
    Xt[::17, 3] = np.nan
    clf = cb.CatBoostClassifier(loss_function=loss, iterations=30, depth=4, verbose=False, thread_count=1, random_seed=0)
    clf.fit(Xt, yt)
    path = str(tmp_path / "model.json")
    clf.save_model(path, format="json")
    lm = {i: i for i in range(k)}
    fb = models.Fpt_Boost.from_json(path, lm)
    X = rng.normal(size=(300, K_FPT))
    X[::13, 3] = np.nan
    raw, prob, pred, conf = fb.predict_raw(X)
    raw_cb = np.asarray(clf.predict(X, prediction_type="RawFormulaVal", thread_count=1), dtype=np.float64).reshape(len(X), -1)
    p_cb = clf.predict_proba(X, thread_count=1)
    import json

    with open(path) as fh:
        m = boost_ref.from_json(json.load(fh))
    c = boost_ref.contract(m, X)
    print(f"catboost {loss}: max |raw - RawFormulaVal| {np.abs(raw - raw_cb).max():.3g}, restatement "
          f"{np.abs(c['raw'] - raw_cb).max():.3g}; max |p - predict_proba| {np.abs(prob - p_cb).max():.3g}, T {c['T']:.3g}")
    assert np.array_equal(c["raw"], raw_cb) and np.array_equal(raw, raw_cb)
    assert np.abs(p_cb.astype(np.longdouble) - c["p_ex"]).max() <= c["T"] and np.abs(prob - p_cb).max() <= 2 * c["T"]
    assert np.array_equal(pred[~c["close"]], np.argmax(p_cb, axis=1)[~c["close"]])
    wrapped = models.from_reference(type("Fpt_Boost", (), dict(model=clf, label_mapper=lm, thresholds=None, n_classes=k,
                                                                noise_class=False))())
    assert np.array_equal(wrapped.predict_raw(X)[0], raw)
