"""N1: the classifier tail of DTW_SVM.predict -- kernel value exp(-gamma d^p), one-vs-one decision sums,
Platt sigmoids, libsvm's pairwise coupling, process_probs -- pinned exactly over its model domain and on all three device
kernels (svm_predict_mfma_kernel, svm_predict_kernel behind WDX_OPT_SVM_SCALAR, the fused DTW epilogue + svm_finish).

Exact tier: every distance is 0 or far enough that gamma d^p >= 110, so every kernel value is exactly 1 or exactly 0 in
float32 on the device (-fno-fast-math) and in NumPy alike; what follows is float64 that differs from the oracle's libsvm
restatement only in summation order and exp / division rounding, so probabilities are compared at 1e-12.  Reads whose
coupling stops within rounding of its tolerance (helper margin, tests/helpers/svm_ref.py) are excluded by rule and
counted.  The tests that run real DTW distances (float32 exp: one ulp apart from NumPy) compare the device forms with
one another at 1e-12 and with the oracle at 1e-5."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import svm_ref
from oracle import wdx_oracle as orc
from warpdemux_amd import _lib, sig_proc, synth

pytestmark = pytest.mark.gpu

MARGIN_EXACT = 1e-8     # stopping-margin rule of the exact tier (K identical on both sides)
MARGIN_FLOAT32 = 1e-5   # ... of comparisons whose kernel values may differ by one float32 ulp
READ_COUNTS = (1, 15, 16, 17)   # partial 16-read tiles, checked against the rows of the full 1043-read call
N_READS = 1043


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _engine(refs):
    from warpdemux_amd.engine import DemuxEngine

    return DemuxEngine(refs, 15, 0.1, sig_proc.SegParams(barcode_num_events=refs.shape[1]))


def _predict(eng, Dd, scalar):
    eng.ctx.set_option(_lib.OPT_SVM_SCALAR, int(scalar))
    try:
        return tuple(t.cpu().numpy() for t in eng.svm_predict(Dd))
    finally:
        eng.ctx.set_option(_lib.OPT_SVM_SCALAR, 0)


@functools.lru_cache(maxsize=None)
def _exact_case(k):
    """model k of the grid (n_support cycling through 1..5, 63..65, 127..129; (p, gamma) cycling), its 0 / far distances
    and the reference side: helper + oracle on K = (D == 0)"""
    p, gamma, far = svm_ref.EXACT_KERNELS[k % len(svm_ref.EXACT_KERNELS)]
    m = svm_ref.synth_model(k, seed=k, thresholds=k % 2 == 0, gamma=gamma, pwr_dist=p)
    D = svm_ref.exact_distances(N_READS, m.n_train, far, seed=1000 + k)
    K = (D == 0).astype(np.float64)
    return m, D, m.predict(K), orc.svm_predict_proba(K, *m.arrays())


def _check_exact(m, ref, prob_o, got, what):
    """the exact tier's assertions of one device output (prob, pred, conf) against the oracle / helper"""
    prob, pred, conf = got
    use = ref.margin >= MARGIN_EXACT
    assert (~use).mean() < 0.01, f"{what}: {(~use).sum()} reads within the stopping margin"
    np.testing.assert_allclose(prob[use], prob_o[use], rtol=0, atol=1e-12, err_msg=what)
    srt = np.sort(prob_o, axis=1)
    np.testing.assert_allclose(conf[use], (srt[:, -1] - srt[:, -2])[use], rtol=0, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(prob.sum(axis=1), 1.0, rtol=0, atol=1e-12, err_msg=what)
    far = ref.conf > 1e-9
    if m.thresholds is not None:
        far &= np.abs(ref.conf - m.thresholds[np.argmax(ref.prob, axis=1)]) > 1e-9
    assert far.mean() > 0.95 and np.array_equal(pred[use & far], ref.pred[use & far]), what
    return use


@pytest.mark.parametrize("k", range(2, 17))
def test_exact_tier_matrix_core_and_scalar_kernels_vs_oracle(k):
    """Both distance-matrix kernels against the oracle at 1e-12 on 0 / 1 kernel values, every k of 2..16, p = 1, 2, 3,
    gamma != 1, thresholds and none; read counts 1, 15, 16, 17 give the bits of the full call's rows."""
    import torch

    m, D, ref, prob_o = _exact_case(k)
    p, gamma = m.pwr_dist, m.gamma
    # the reference's own float32 formula (models/dtw_svm.py:21-22) yields exactly 0 / 1 on these distances
    Kref = np.exp(-gamma * np.power(D, p))
    assert Kref.dtype == np.float32 and np.array_equal(Kref, (D == 0).astype(np.float32))
    eng = _engine(np.zeros((m.n_train, 25)))
    try:
        eng.set_svm(m.to_dtw_svm(np.zeros((m.n_train, 25))))
        Dd = torch.from_numpy(D).to(eng.tdev)
        full = {}
        for scalar in (False, True):
            what = f"k={k} {'scalar' if scalar else 'mfma'}"
            full[scalar] = _predict(eng, Dd, scalar)
            use = _check_exact(m, ref, prob_o, full[scalar], what)
            for n in READ_COUNTS:
                part = _predict(eng, Dd[:n], scalar)
                assert all(_same(a, b[:n]) for a, b in zip(part, full[scalar])), f"{what}: {n} reads"
        np.testing.assert_allclose(full[False][0][use], full[True][0][use], rtol=0, atol=1e-12)
        np.testing.assert_allclose(full[False][2][use], full[True][2][use], rtol=0, atol=1e-12)
    finally:
        eng.close()


def test_exact_tier_grid_reaches_both_clips_and_both_sigmoid_branches():
    """the grid above exercises min_prob on both sides and both branches of sigmoid_predict"""
    sig = np.concatenate([_exact_case(k)[2].sigmoid.ravel() for k in range(2, 17)])
    fApB = np.concatenate([_exact_case(k)[2].fApB.ravel() for k in range(2, 17)])
    assert (sig < svm_ref.MIN_PROB).sum() > 100 and (sig > 1 - svm_ref.MIN_PROB).sum() > 100
    assert (fApB >= 0).sum() > 1000 and (fApB < 0).sum() > 1000
    excluded = sum(int((_exact_case(k)[2].margin < MARGIN_EXACT).sum()) for k in range(2, 17))
    assert excluded < 0.002 * 15 * N_READS


@pytest.mark.parametrize("scalar", [False, True])
def test_exact_tier_resolves_one_support_vector(scalar):
    """Positive control: one dual coefficient moved by 1e-8 -- the LAST vector of a class with n_support % 4 == 1 (the
    tail of the matrix-core kernel's 4-vector step) -- must fail the 1e-12 comparison on the reads whose kernel value
    hits that vector (every read where the helper sees the change), and on no other read."""
    import torch

    m, D, ref, prob_o = _exact_case(5)
    c = max((c for c in range(m.k) if m.n_support[c] % 4 == 1), key=lambda c: m.n_support[c])
    s = int(np.sum(m.n_support[:c]) + m.n_support[c] - 1)
    bad = svm_ref.synth_model(m.k, seed=m.k, thresholds=m.thresholds is not None, gamma=m.gamma, pwr_dist=m.pwr_dist)
    bad.dual_coef = bad.dual_coef.copy()
    bad.dual_coef[0, s] += 1e-8
    K = (D == 0).astype(np.float64)
    moved = np.abs(bad.predict(K).prob - ref.prob).max(axis=1)
    hit = D[:, m.support[s]] == 0
    use = ref.margin >= MARGIN_EXACT
    sens = use & (moved > 1e-11)
    assert not (moved[~hit] > 0).any() and sens.sum() > 0.3 * hit.sum() > 10
    eng = _engine(np.zeros((m.n_train, 25)))
    try:
        eng.set_svm(bad.to_dtw_svm(np.zeros((m.n_train, 25))))
        prob = _predict(eng, torch.from_numpy(D).to(eng.tdev), scalar)[0]
    finally:
        eng.close()
    err = np.abs(prob - prob_o).max(axis=1)
    assert (err[sens] > 1e-12).all(), f"{(err[sens] <= 1e-12).sum()} of {sens.sum()} perturbed reads not resolved"
    assert (err[use & ~hit] <= 1e-12).all()


def test_exact_tier_large_model_scalar_refuses_matrix_core_matches():
    """~19 500 support vectors: beyond the scalar kernel's LDS carve-up (refused with an error, nothing launched); the
    matrix-core kernel streams them and still matches the oracle at 1e-12."""
    import torch

    p, gamma, far = svm_ref.EXACT_KERNELS[0]
    m = svm_ref.synth_model(3, seed=77, n_support=[6499, 6500, 6501], n_extra=500, thresholds=True, gamma=gamma,
                            pwr_dist=p)
    m.dual_coef = m.dual_coef * 0.02       # decision values of order one: not every sigmoid clipped
    D = svm_ref.exact_distances(64, m.n_train, far, seed=78)
    K = (D == 0).astype(np.float64)
    ref, prob_o = m.predict(K), orc.svm_predict_proba(K, *m.arrays())
    assert (np.abs(ref.sigmoid - 0.5) < 0.49).mean() > 0.3
    eng = _engine(np.zeros((m.n_train, 25)))
    try:
        eng.set_svm(m.to_dtw_svm(np.zeros((m.n_train, 25))))
        Dd = torch.from_numpy(D).to(eng.tdev)
        with pytest.raises(NotImplementedError, match="too large"):
            _predict(eng, Dd, True)
        _check_exact(m, ref, prob_o, _predict(eng, Dd, False), "large model, mfma")
    finally:
        eng.close()


# ------------------------------------------------------------------- fused form (DTW epilogue) over the model domain ----

def _training_fingerprints(eng0, spec, n_train):
    """fingerprints of synthetic reads as the training set (real DTW distances between reads and references)"""
    sig, off, a_s, a_e, _, max_len = eng0.synth_packed(spec, 50_000, n_train + 200)
    fpt, _, _, st = eng0.fingerprint(sig, a_s, a_e, offsets=off, max_len=max_len, want_stats=False)
    fpt, st = fpt.cpu().numpy(), st.cpu().numpy()
    X = fpt[st == 0][:n_train]
    assert X.shape[0] == n_train
    return np.ascontiguousarray(X)


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("k", [2, 9, 16])
def test_fused_form_over_the_model_domain(k, p):
    """wdx_demux_svm_dev's fused form (decision sums in the DTW epilogue, two chunks per class: a 1-vector class leaves
    the second chunk empty), the row-block form and the row-block form on the scalar kernel: pwr 1 / 2 / 3 with gamma
    putting the median kernel value in (1e-3, 0.5), no thresholds.  The three agree at 1e-12, each matches the oracle
    at 1e-5 on a sample, failed reads are masked in every form."""
    import torch

    cyc = svm_ref.N_SUPPORT_CYCLE
    n_support = [1, 65] if k == 2 else [cyc[c % len(cyc)] for c in range(k)]
    m = svm_ref.synth_model(k, seed=10 * k + p, n_support=n_support, thresholds=False, pwr_dist=p)
    assert 1 in m.n_support and any(c % 2 == 1 and c > 1 for c in m.n_support)
    spec = synth.SynthSpec(n_barcodes=4)
    eng0 = _engine(np.zeros((4, 25)))
    try:
        X = _training_fingerprints(eng0, spec, m.n_train)
    finally:
        eng0.close()
    eng = _engine(X)
    try:
        n = 1024
        sig, off, a_s, a_e, _, max_len = eng.synth_packed(spec, 7000, n)
        a_e = a_e.clone()
        a_e[::97] = a_s[::97] + 40                  # a few reads that fail
        fpt, _, _, _ = eng.fingerprint(sig, a_s, a_e, offsets=off, max_len=max_len, want_stats=False)
        D0 = eng.dtw(fpt[:256], want_argmin=False)[0].cpu().numpy()
        med = float(np.median(D0[np.isfinite(D0)]))
        m.gamma = float(np.float32(1.5 / med ** p))        # median kernel value ~ exp(-1.5)
        eng.set_svm(m.to_dtw_svm(X))
        forms = {}
        forms["fused"] = eng.demux_svm(sig, a_s, a_e, offsets=off, max_len=max_len)
        forms["rows"] = eng.demux_svm(sig, a_s, a_e, offsets=off, max_len=max_len, want_dist=True)
        eng.ctx.set_option(_lib.OPT_SVM_SCALAR, 1)
        try:
            forms["scalar"] = eng.demux_svm(sig, a_s, a_e, offsets=off, max_len=max_len, want_dist=True)
        finally:
            eng.ctx.set_option(_lib.OPT_SVM_SCALAR, 0)
        out = {f: [None if t is None else t.cpu().numpy() for t in v] for f, v in forms.items()}
    finally:
        eng.close()
    status = out["rows"][3]
    ok = status == 0
    dist = out["rows"][4]
    assert (~ok).sum() >= 5 and ok.sum() > 0.9 * n
    Kf = np.exp(-m.gamma * np.power(dist[ok], p))
    assert Kf.dtype == np.float32 and 1e-3 < np.median(Kf) < 0.5
    ref = m.predict(Kf)
    use = ref.margin >= MARGIN_FLOAT32
    print(f"k={k} p={p}: {(~use).sum()} of {ok.sum()} reads within the stopping margin")
    assert (~use).sum() <= max(3, 0.01 * ok.sum())
    base = out["rows"]
    for f, (prob, pred, conf, st, _, _) in out.items():
        assert np.array_equal(st, status), f
        assert (pred[~ok] == -1).all() and np.isnan(prob[~ok]).all() and np.isnan(conf[~ok]).all(), f
        np.testing.assert_allclose(prob[ok][use], base[0][ok][use], rtol=0, atol=1e-12, err_msg=f)
        np.testing.assert_allclose(conf[ok][use], base[2][ok][use], rtol=0, atol=1e-12, err_msg=f)
        np.testing.assert_allclose(prob[ok].sum(axis=1), 1.0, rtol=0, atol=1e-12, err_msg=f)
        far = use & (ref.conf > 1e-9)
        assert np.array_equal(pred[ok][far], base[1][ok][far]), f
    # against the oracle's fingerprints + DTW + libsvm restatement on a sample (float32 exp: 1e-5)
    ns = 200
    o = off[: ns + 1].cpu().numpy()
    ofp, _, _, ost = orc.fingerprint_packed(sig[: int(o[-1])].cpu().numpy(), o, a_s[:ns].cpu().numpy(),
                                            a_e[:ns].cpu().numpy(), orc.SegParams(barcode_num_events=25))
    assert np.array_equal(ost, status[:ns])
    oko = ost == 0
    Ko = np.exp(-m.gamma * np.power(orc.dtw_matrix(ofp[oko], X, 15, 0.1), p))
    prob_o = orc.svm_predict_proba(Ko, *m.arrays())
    mo = m.predict(Ko).margin >= MARGIN_FLOAT32
    for f, v in out.items():
        np.testing.assert_allclose(v[0][:ns][oko][mo], prob_o[mo], rtol=0, atol=1e-5, err_msg=f)


# ------------------------------------------------------------------------------- host entry: chunks and validation ----

def test_dtw_svm_predict_crosses_its_row_chunks():
    """wdx_dtw_svm_predict runs 2^30 / (4 nY) rows per pass: 16 384 references and 40 000 queries take three passes;
    the result is the bits of eng.dtw + eng.svm_predict on the same rows."""
    import torch

    nY, n = 16384, 40000
    assert -(-n // ((1 << 30) // (4 * nY))) == 3
    m = svm_ref.synth_model(4, seed=5, n_support=[100, 37, 64, 129], n_extra=nY - 330, thresholds=False, gamma=0.05,
                            pwr_dist=2)         # median kernel value ~0.4
    rng = np.random.default_rng(6)
    X = rng.normal(size=(nY, 25))
    Xq = X[rng.integers(0, nY, n)] + 0.5 * rng.normal(size=(n, 25))
    model = m.to_dtw_svm(X)
    pred, prob = model.predict(Xq)
    eng = _engine(X)
    try:
        eng.set_svm(model)
        d, _ = eng.dtw(torch.from_numpy(Xq).to(eng.tdev), want_argmin=False)
        p2, q2, _ = (t.cpu().numpy() for t in eng.svm_predict(d))
    finally:
        eng.close()
    assert _same(prob, p2) and np.array_equal(pred, q2.astype(np.int64))
    assert np.ptp(prob, axis=0).min() > 0.01


def _model_c(m, **over):
    """wdx_svm_model of a SynthModel with fields overridden (the arrays are kept alive in the returned tuple)"""
    arrs = dict(n_support=np.array(m.n_support, dtype=np.int32), support=np.array(m.support, dtype=np.int32),
                dual_coef=np.ascontiguousarray(m.dual_coef), rho=m.rho, probA=m.probA, probB=m.probB,
                label_map=m.label_map, thresholds=m.thresholds)
    scal = dict(n_classes=m.k, n_sv=int(m.n_support.sum()), n_train=m.n_train, pwr_dist=m.pwr_dist, gamma=m.gamma)
    for key, v in over.items():
        (arrs if isinstance(v, np.ndarray) else scal)[key] = v
    c = _lib.SvmModelC(scal["n_classes"], scal["n_sv"], scal["n_train"], scal["pwr_dist"], scal["gamma"],
                       *[None if arrs[f] is None else arrs[f].ctypes.data for f in
                         ("n_support", "support", "dual_coef", "rho", "probA", "probB", "label_map", "thresholds")])
    return c, arrs


def test_svm_set_model_refuses_bad_models_and_keeps_the_previous_one():
    import torch

    p, gamma, far = svm_ref.EXACT_KERNELS[2]
    m = svm_ref.synth_model(5, seed=5, gamma=gamma, pwr_dist=p)
    D = svm_ref.exact_distances(100, m.n_train, far, seed=9)
    eng = _engine(np.zeros((m.n_train, 25)))
    L = _lib.load()
    try:
        eng.set_svm(m.to_dtw_svm(np.zeros((m.n_train, 25))))
        Dd = torch.from_numpy(D).to(eng.tdev)
        before = _predict(eng, Dd, False)
        neg = m.n_support.copy()
        neg[1] = -neg[1]
        short = m.n_support.copy()
        short[0] += 1
        sup_hi, sup_lo = m.support.copy(), m.support.copy()
        sup_hi[-1] = m.n_train
        sup_lo[3] = -1
        big = np.ones(17, dtype=np.int32)
        bad = {"k=1": dict(n_classes=1), "k=17": dict(n_classes=17, n_support=big, n_sv=17),
               "negative n_support": dict(n_support=neg), "sum(n_support) != n_sv": dict(n_support=short),
               "support >= n_train": dict(support=sup_hi), "support < 0": dict(support=sup_lo), "pwr_dist=0": dict(pwr_dist=0)}
        for what, over in bad.items():
            c, keep = _model_c(m, **over)
            rc = L.wdx_svm_set_model(eng.ctx.handle, C.byref(c))
            assert rc == _lib.WDX_ERR_INVALID, what
            assert len(L.wdx_last_error().decode()) > 0, what
            after = _predict(eng, Dd, False)
            assert all(_same(a, b) for a, b in zip(before, after)), what
        c, keep = _model_c(m)
        _lib.check(L.wdx_svm_set_model(eng.ctx.handle, C.byref(c)))     # the same model through the raw ABI: same bits
        assert all(_same(a, b) for a, b in zip(before, _predict(eng, Dd, False)))
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------- live tick with a model ----

def test_live_tick_masks_failed_reads_like_the_other_entry_points():
    """wdx_live_tick with use_svm: a read whose fingerprint failed comes back with pred -1 and NaN prob / conf through the
    C ABI itself (as wdx_demux_svm_dev and the minibatch path return them), not with the tail's output on NaN distances."""
    from test_gpu_live import _ragged_rows, _svm_model
    from warpdemux_amd.live import LiveDemux

    model, _ = _svm_model()
    ld = LiveDemux(model=model, max_reads=32, max_samples=9000)
    try:
        n, k = 12, model.n_classes
        rows = _ragged_rows(synth.SynthSpec(n_barcodes=4), 96_000, n)
        a_s = np.zeros(n, np.int32)
        a_e = np.array([r.size - 100 for r in rows], dtype=np.int32)
        rows[2] = np.full(1400, 80.0, dtype=np.float32)     # constant: no change-points -> failed read
        a_e[2] = 1400
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in rows])
        ln = np.array([r.size for r in rows], dtype=np.int32)
        pc = ld.params.to_c()
        status, call = np.zeros(n, np.int32), np.zeros(n, np.int32)
        prob, pred, conf = np.zeros((n, k)), np.zeros(n, np.int32), np.zeros(n)
        fpt = np.zeros((n, 25))
        okf = np.ones(n, np.uint8)
        okf[7] = 0                                          # rejected by the caller -> status 1
        _lib.check(ld.L.wdx_live_tick(ld.ctx.handle, ptrs, _lib.ptr(ln), n, _lib.ptr(a_s), _lib.ptr(a_e), _lib.ptr(okf), C.byref(pc),
                                      ld.nY, 1, _lib.ptr(fpt), None, _lib.ptr(call), _lib.ptr(status), _lib.ptr(prob),
                                      _lib.ptr(pred), _lib.ptr(conf)))
        bad = status != 0
        assert bad[2] and bad[7] and (~bad).sum() >= n - 4
        assert (pred[bad] == -1).all() and np.isnan(prob[bad]).all() and np.isnan(conf[bad]).all()
        assert np.isfinite(prob[~bad]).all() and np.isfinite(conf[~bad]).all()
        y_pred, y_prob = model.predict(fpt[~bad], nproc=1)
        assert _same(prob[~bad], y_prob) and np.array_equal(pred[~bad], y_pred)
    finally:
        ld.close()
