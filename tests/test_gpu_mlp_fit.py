"""The device MLP trainer (include/wdx.h: wdx_mlp_fit_device, wdx_mlp_fit; DemuxEngine.mlp_fit; models.DTW_MLP.fit(solver="device"))
against scikit-learn on the same initial weights and the same epoch orders.

Accuracy contract per case (it follows DESIGN.md 4.7's): the exact run is scikit-learn in float64 on the scaled float32 input widened;
E_ref = max |scikit-learn float32 - exact| over all parameters; the device must stay within T = 4 max(E_ref, u max|theta|) of the
exact run on every parameter, u = 2^-24.  The loss curve is held the same way (E_ref, max |loss| and T of its own).  Every case
prints its figures before it asserts; `measure` returns them (tools/bench_mlp_fit.py writes profiles/mlp_fit_accuracy.json).

The shapes are the smallest at which a kernel takes another path: a last batch of 11 rows (no multiple of 16 or 4); one logistic
output unit behind two hidden layers; every dimension a whole tile; 16 classes with batch 1 and with a batch beyond m; a fan-in of
2 601 (the long k chain); each of the four activations; no shuffling; no scaler; a leading dimension beyond F.  Beyond these twelve,
22 cases (34 in all) run the rest of the accepted domain: seven at its edges (five weight matrices, hidden widths 1, 3, 5 and 512,
the step from four to five tiles, every dimension 1, a batch of WDX_MLP_FIT_MAX_BATCH rows), six with a hyper-parameter away from
scikit-learn's default (HYPER), and nine that read the gradient out (RO: see there and tests/test_mlp_fit_readout_host.py).  A fit
whose loss is not finite ends with its state."""
import ctypes as C
import functools
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import mlp_ref  # noqa: E402

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
SEED = 11

# name: rows, features, hidden, classes, activation, batch, epochs, shuffle, scaler, extra leading dimension
CASES = {
    "203x19-17-5-last-batch-11": (203, 19, (17,), 5, "relu", 64, 6, True, True, 0),
    "530x37-24x10-2-tanh": (530, 37, (24, 10), 2, "tanh", 200, 6, True, True, 0),
    "96x16-16-3-whole-tiles": (96, 16, (16,), 3, "relu", 32, 6, True, True, 0),
    "70x5-3-16-batch-1": (70, 5, (3,), 16, "relu", 1, 6, True, True, 0),
    "70x5-3-16-batch-beyond-m": (70, 5, (3,), 16, "relu", 500, 6, True, True, 0),
    "300x2601-100-10-long-k": (300, 2601, (100,), 10, "relu", 200, 2, True, True, 0),
    "203x19-identity": (203, 19, (17,), 5, "identity", 64, 6, True, True, 0),
    "203x19-logistic": (203, 19, (17,), 5, "logistic", 64, 6, True, True, 0),
    "203x19-tanh": (203, 19, (17,), 5, "tanh", 64, 6, True, True, 0),
    "203x19-unshuffled": (203, 19, (17,), 5, "relu", 64, 6, False, True, 0),
    "203x19-no-scaler": (203, 19, (17,), 5, "relu", 64, 6, True, False, 0),
    "203x19-ld-beyond-F": (203, 19, (17,), 5, "relu", 64, 6, True, True, 13),
}
# name: keyword arguments given both to MLPClassifier and to DemuxEngine.mlp_fit; a case without an entry runs scikit-learn's defaults
HYPER = {}

# The accepted domain beyond the shapes above (default hyper-parameters): five weight matrices with deltas for l = 1 .. 4 and widths
# below four; a hidden layer of one unit; all eight accumulators of a wave and a forward LDS beyond 64 KB; the delta kernel and 1 024
# Adam tiles at 512 x 512; the step from four to five tiles; every dimension 1; WDX_MLP_FIT_MAX_BATCH rows in one chain.
CASES.update({
    "max-depth-relu": (150, 9, (20, 3, 33, 5), 4, "relu", 64, 4, True, True, 0),
    "max-depth-tanh-1unit": (150, 9, (17, 16, 15, 1), 2, "tanh", 64, 4, True, True, 0),
    "width-512": (120, 7, (512,), 3, "relu", 50, 3, True, True, 0),
    "width-512x512-logistic": (100, 5, (512, 512), 16, "logistic", 48, 2, True, True, 0),
    "width-64x65": (90, 6, (64, 65), 3, "relu", 32, 4, True, True, 0),
    "tiny-2x1-1": (2, 1, (1,), 2, "tanh", 1, 6, True, True, 0),
    "batch-1024": (1030, 6, (8,), 3, "relu", 1024, 3, True, True, 0),
})

# Each hyper-parameter alone at a value of its own (two swapped fields cannot cancel), and all five together.
_BASE = (203, 19, (17,), 5, None, 64, 6, True, True, 0)
for _name, _act, _kw in [
    ("alpha-0.5", "relu", dict(alpha=0.5)),
    ("lr-0.02", "relu", dict(learning_rate_init=0.02)),
    ("beta1-0", "tanh", dict(beta_1=0.0)),
    ("beta2-0.9", "tanh", dict(beta_2=0.9)),
    ("epsilon-1e-3", "tanh", dict(epsilon=1e-3)),
    ("hyper-mixed-logistic", "logistic", dict(alpha=0.03, learning_rate_init=0.004, beta_1=0.7, beta_2=0.95, epsilon=1e-5)),
]:
    CASES[_name] = _BASE[:4] + (_act,) + _BASE[5:]
    HYPER[_name] = _kw

# Gradient read-out.  With epsilon = 1e-8 Adam's m / (sqrt(v) + epsilon) does not change when a gradient element is scaled, so the
# cases above cannot see a wrong divisor, a mis-scaled alpha w or a moment carried with the wrong weight
# (tests/test_mlp_fit_readout_host.py measures that blind spot).  Under RO the update is -g / (|g| + 1), monotone in g: the result
# reads out every element of every gradient.  37 rows, 19 -> 17 -> 33: every dimension a ragged tile, nb no multiple of 4.
RO = dict(alpha=0.0, learning_rate_init=1.0, beta_1=0.0, beta_2=0.0, epsilon=1.0)
_RO_BASE = (37, 19, (17, 33), 5, "tanh", 200, 1, True, True, 0)
for _act in ("relu", "tanh", "logistic", "identity"):
    CASES["readout-" + _act] = _RO_BASE[:4] + (_act,) + _RO_BASE[5:]
    HYPER["readout-" + _act] = RO
_MOMENTS = dict(alpha=0.0, learning_rate_init=1.0, beta_1=0.5, beta_2=0.25, epsilon=1.0)
for _name, _spec, _kw in [
    ("readout-1unit-alpha", (37, 19, (17, 33), 2, "tanh", 200, 1, True, True, 0), dict(RO, alpha=0.5)),   # alpha w at full weight
    ("readout-two-steps", (37, 19, (17, 33), 5, "tanh", 26, 1, True, True, 0), RO),   # 26 and 11 rows: the divisor is nb
    ("readout-moments", (37, 19, (17, 33), 5, "tanh", 26, 2, True, True, 0), _MOMENTS),   # both moments at visible weight
    ("readout-moments-alpha", (37, 19, (17, 33), 5, "logistic", 26, 2, True, True, 0), dict(_MOMENTS, alpha=0.5, learning_rate_init=0.25)),
    ("readout-batch-1024", (1030, 6, (8,), 3, "tanh", 1024, 1, True, True, 0), RO),   # the 1 024-row chain
]:
    CASES[_name] = _spec
    HYPER[_name] = _kw


def _imports():
    global torch, _lib, _mlp_fit, models, DemuxEngine
    import torch
    from warpdemux_amd import _lib, _mlp_fit, models
    from warpdemux_amd.engine import DemuxEngine


@pytest.fixture(scope="module")
def eng():
    _imports()
    e = DemuxEngine(np.random.default_rng(0).normal(size=(4, 25)), 15, 0.1)
    yield e
    e.close()


def distances(m, F, k, seed=0, sigma=3.0):
    """(float32 (m, F) distances around per-class centres, class index per row; every class occurs)"""
    rng = np.random.default_rng(1000 * seed + m + F)
    centres = rng.uniform(2, 8, size=(k, F))
    y = rng.integers(0, k, size=m)
    y[:k] = np.arange(k)
    return np.abs(centres[y] + rng.normal(0, sigma, size=(m, F))).astype(np.float32), y.astype(np.int32)


def scaler_of(D):
    from sklearn.preprocessing import StandardScaler

    s = StandardScaler().fit(D)
    return s.mean_, s.scale_


def sklearn_fit(X, y, hidden, act, batch, epochs, shuffle, seed=SEED, **kw):
    from sklearn.neural_network import MLPClassifier

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return MLPClassifier(hidden_layer_sizes=hidden, activation=act, batch_size=batch, shuffle=shuffle, max_iter=epochs, random_state=seed,
                             **kw).fit(X, y)


def _flat(coefs, intercepts):
    return np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in list(coefs) + list(intercepts)])


def reference(name):
    """The case's inputs and both scikit-learn runs, computed once and shared: the exact run (float64) and the float32 run."""
    return reference_of(CASES[name], tuple(sorted(HYPER.get(name, {}).items())))


@functools.lru_cache(maxsize=None)
def reference_of(spec, hyper=()):
    """`reference` of a case given as its tuple and its sorted hyper-parameter items"""
    m, F, hidden, k, act, batch, epochs, shuffle, scaled, _ = spec
    D, y = distances(m, F, k)
    mean, scale = scaler_of(D) if scaled else (None, None)
    Xs = mlp_ref.scale([(mean, scale)], D)
    sk64 = sklearn_fit(Xs.astype(np.float64), y, hidden, act, batch, epochs, shuffle, **dict(hyper))
    sk32 = sklearn_fit(Xs, y, hidden, act, batch, epochs, shuffle, **dict(hyper))
    assert sk32.coefs_[0].dtype == np.float32 and sk64.coefs_[0].dtype == np.float64
    th64, th32 = _flat(sk64.coefs_, sk64.intercepts_), _flat(sk32.coefs_, sk32.intercepts_)
    l64, l32 = np.asarray(sk64.loss_curve_, np.float64), np.asarray(sk32.loss_curve_, np.float64)
    e_ref, e_loss = float(np.abs(th32 - th64).max()), float(np.abs(l32 - l64).max())
    for a in (D, y, th64, l64):
        a.setflags(write=False)
    return dict(D=D, y=y, mean=mean, scale=scale, th64=th64, l64=l64, e_ref=e_ref, e_loss=e_loss,
                T=4 * max(e_ref, U32 * float(np.abs(th64).max())), T_loss=4 * max(e_loss, U32 * float(np.abs(l64).max())), n_iter=sk64.n_iter_)


def device_fit(eng, name, **over):
    m, F, hidden, k, act, batch, epochs, shuffle, scaled, ld_extra = CASES[name]
    R = reference(name)
    sizes = _mlp_fit.layer_sizes(F, hidden, k)
    W0, B0, order = _mlp_fit.schedule(sizes, act, SEED, m, epochs, shuffle)
    wide = torch.full((m, F + ld_extra), float("nan"), dtype=torch.float32, device=eng.tdev)
    wide[:, :F] = torch.from_numpy(np.array(R["D"])).to(eng.tdev)
    kw = dict(activation=act, n_classes=k, mean=R["mean"], scale=R["scale"], order=order, batch_size=batch, max_epochs=epochs)
    kw.update(HYPER.get(name, {}))
    kw.update(over)
    return eng.mlp_fit(wide[:, :F], torch.from_numpy(np.array(R["y"])).to(eng.tdev), W0, B0, **kw)


def measure(eng, name):
    """the case's figures: E_ref, T, the device's error and its ratio to E_ref, for the parameters and for the loss curve"""
    R = reference(name)
    res = device_fit(eng, name)
    th = _flat(res.coefs, res.intercepts)
    err = float(np.abs(th - R["th64"]).max())
    ok_len = len(res.loss_curve) == len(R["l64"])
    err_loss = float(np.abs(res.loss_curve - R["l64"]).max()) if ok_len else float("nan")
    return dict(case=name, e_ref=R["e_ref"], max_abs_theta=float(np.abs(R["th64"]).max()), T=R["T"], device_err=err,
                ratio_to_e_ref=err / R["e_ref"] if R["e_ref"] else float("nan"), ratio_to_T=err / R["T"], e_ref_loss=R["e_loss"],
                T_loss=R["T_loss"], device_err_loss=err_loss, ratio_loss=err_loss / R["e_loss"] if R["e_loss"] else float("nan"),
                ratio_loss_to_T=err_loss / R["T_loss"], hyper=dict(HYPER.get(name, {})), n_iter=res.n_iter,
                state=res.state, finite=bool(np.isfinite(th).all()), float32=all(a.dtype == np.float32 for a in res.coefs + res.intercepts))


@pytest.mark.parametrize("name", list(CASES))
def test_device_follows_scikit_learn_within_the_contract(eng, name):
    f = measure(eng, name)
    print(f"{name}: E_ref {f['e_ref']:.3g} T {f['T']:.3g} device {f['device_err']:.3g} (x{f['ratio_to_e_ref']:.3g} E_ref) | loss: E_ref "
          f"{f['e_ref_loss']:.3g} T {f['T_loss']:.3g} device {f['device_err_loss']:.3g} (x{f['ratio_loss']:.3g})")
    assert f["finite"] and f["float32"] and f["state"] == "max_epochs" and f["n_iter"] == CASES[name][6] == reference(name)["n_iter"]
    assert f["device_err"] <= f["T"], f
    assert f["device_err_loss"] <= f["T_loss"], f


def test_two_fits_of_the_same_inputs_are_bitwise_equal(eng):
    for name in ("203x19-17-5-last-batch-11", "530x37-24x10-2-tanh"):
        a, b = device_fit(eng, name), device_fit(eng, name)
        for x, y in zip(a.coefs + a.intercepts, b.coefs + b.intercepts):
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), name
        assert np.array_equal(a.loss_curve.view(np.int64), b.loss_curve.view(np.int64)) and a.n_iter == b.n_iter


def test_host_form_equals_the_device_form(eng):
    """wdx_mlp_fit on the host matrix (its own upload, the context's own stream) returns the bits of DemuxEngine.mlp_fit"""
    name = "203x19-17-5-last-batch-11"
    m, F, hidden, k, act, batch, epochs, shuffle, _, _ = CASES[name]
    R = reference(name)
    sizes = _mlp_fit.layer_sizes(F, hidden, k)
    W0, B0, order = _mlp_fit.schedule(sizes, act, SEED, m, epochs, shuffle)
    p = _mlp_fit.params_c(sizes, act, k, batch, epochs, 10, 1e-3, 1e-4, 0.9, 0.999, 1e-8, 1e-4)
    W, B, mean, scale, order = _mlp_fit.check_arrays(sizes, m, W0, B0, R["mean"], R["scale"], order, epochs)
    host = _mlp_fit.fit_host(np.array(R["D"]), np.array(R["y"]), p, W, B, mean, scale, order)
    dev = device_fit(eng, name)
    for x, y in zip(host.coefs + host.intercepts, dev.coefs + dev.intercepts):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    assert np.array_equal(host.loss_curve, dev.loss_curve) and host.state == dev.state == "max_epochs"


def test_kernel_time_counts_the_launches(eng):
    name = "530x37-24x10-2-tanh"
    eng.kernel_timing(True)
    try:
        eng.kernel_time_reset()
        device_fit(eng, name)
        ms, launches = eng.kernel_time(_lib.K_MLP_FIT)
    finally:
        eng.kernel_timing(False)
    m, batch, epochs, nl = 530, 200, 6, 3
    assert launches == epochs * -(-m // batch) * 2 * nl and ms > 0, (ms, launches)


def test_kernel_time_counts_the_launches_of_five_layers(eng):
    name = "max-depth-relu"
    eng.kernel_timing(True)
    try:
        eng.kernel_time_reset()
        device_fit(eng, name)
        ms, launches = eng.kernel_time(_lib.K_MLP_FIT)
    finally:
        eng.kernel_timing(False)
    m, _, hidden, _, _, batch, epochs = CASES[name][:7]
    nl = len(hidden) + 1
    assert nl == _lib.MLP_MAX_LAYERS == 5 and launches == epochs * -(-m // batch) * 2 * nl == 120 and ms > 0, (ms, launches)


# ---- a model served as fitted ---------------------------------------------------------------------------------------------------------

def _sklearn_twin(dm, D, k):
    """a scikit-learn pipeline carrying the fitted model's scaler and weights"""
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler

    mlp = mlp_ref.random_mlp(D.shape[1], tuple(w.shape[1] for w in dm._coefs[:-1]), k, np.float32, dm.activation, seed=0)
    mlp.coefs_, mlp.intercepts_ = [w.copy() for w in dm._coefs], [b.copy() for b in dm._intercepts]
    s = StandardScaler().fit(D)
    s.mean_, s.scale_ = dm._scalers[0]
    return Pipeline([("scaler", s), ("mlp", mlp)])


def test_a_fitted_model_is_served_as_fitted():
    """DTW_MLP.fit(solver="device") on fingerprints of synthetic reads, then `predict` and `demux_mlp`: the probabilities of
    scikit-learn's predict_proba on the fitted weights, under the tail's contract (tests/helpers/mlp_ref.py)"""
    _imports()
    from warpdemux_amd import sig_proc, synth

    n, L, k = 320, 25, 4
    spec = synth.SynthSpec(n_barcodes=k, seed=5)
    mb, a_s, a_e, bc = synth.generate_minibatch(spec, 0, n, 8000)
    sig = torch.from_numpy(mb).to("cuda")
    a_s, a_e = torch.from_numpy(a_s.astype(np.int32)).to("cuda"), torch.from_numpy(a_e.astype(np.int32)).to("cuda")
    sp = sig_proc.SegParams(barcode_num_events=L)
    probe = DemuxEngine(np.zeros((1, L)), 15, 0.1, sp)
    fpt, _, _, st = probe.fingerprint(sig, a_s, a_e, stride=mb.shape[1], max_len=mb.shape[1])
    probe.close()
    status = st.cpu().numpy()
    X, y = fpt.cpu().numpy(), np.asarray(bc).astype(np.int64)
    good = status == 0
    assert good.sum() > 200 and np.unique(y[good]).size == k
    refs = X[good][:40] + 0.01
    thr = np.array([0.1, 0.2, 0.3, 0.4])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        dm = models.DTW_MLP.fit(X, y * 3 + 1, 15, 0.1, refs=refs, hidden_layer_sizes=(20,), max_iter=8, status=status, thresholds=thr,
                                random_state=3, solver="device")
    assert dm.n_dropped_ == int((~good).sum()) and dm.n_iter_ == 8 and len(dm.loss_curve_) == 8 and dm.loss_curve_[-1] < dm.loss_curve_[0]
    assert dm.dtype == np.float32 and dm.label_mapper == {i: 3 * i + 1 for i in range(k)}
    eng = DemuxEngine(refs, 15, 0.1, sp)
    try:
        eng.set_mlp(dm)
        prob, pred, conf, status2, dist, _ = (t.cpu().numpy() if t is not None else None for t in eng.demux_mlp(
            sig, a_s, a_e, stride=mb.shape[1], max_len=mb.shape[1], want_dist=True, want_fpt=True))
        assert np.array_equal(status2, status)
        D = dist[good]
        est = _sklearn_twin(dm, D, k)
        ref = mlp_ref.DTW_MLP(est, refs, dm.label_mapper, thr, window=15, penalty=0.1)
        c = mlp_ref.contract(est, D, thr)
        pred_sk, _ = mlp_ref.process_probs(c["p_sk"], ref.label_mapper, thr)
        err, bad = mlp_ref.check_outputs(c, prob[good], conf[good], pred[good], pred_sk, np.float32)
        print(f"served: E_ref {c['e_ref']:.3g} T {c['T']:.3g} device err {err:.3g}, accuracy {np.mean(pred[good] == y[good] * 3 + 1):.3f}")
        assert not bad, bad
        y_pred, y_prob = dm.predict(np.ascontiguousarray(X[good]), nproc=1)
        assert np.array_equal(y_prob.astype(np.float64), prob[good]) and np.array_equal(y_pred, pred[good].astype(np.int64))
    finally:
        eng.close()


# ---- held-out accuracy ----------------------------------------------------------------------------------------------------------------

def test_held_out_accuracy_is_that_of_the_host_fit():
    """templates + noise, 10 labels, barycenter references: device and scikit-learn fits with the same seed call the held-out rows
    within one read per hundred of each other"""
    _imports()
    from warpdemux_amd import parallel_distances as pd

    rng = np.random.default_rng(21)
    k, L, n_train, n_test = 10, 25, 800, 500
    templates = rng.normal(size=(k, L))
    y = rng.integers(0, k, n_train + n_test)
    X = templates[y] + rng.normal(0, 0.4, size=(len(y), L))
    Xtr, ytr, Xte, yte = X[:n_train], y[:n_train], X[n_train:], y[n_train:]
    refs = pd.label_barycenters(Xtr, ytr.astype(np.int32), k, window=15, penalty=0.1, n_iter=3)[0]
    D = pd.distance_matrix_to(Xtr, refs, window=15, penalty=0.1, n_jobs=1)
    acc = {}
    for solver in ("device", "sklearn"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            dm = models.DTW_MLP.fit(Xtr, ytr, 15, 0.1, refs=refs, hidden_layer_sizes=(32,), max_iter=40, random_state=4, distances=D,
                                    solver=solver)
        assert dm.dtype == np.float32 and dm.n_iter_ == 40
        y_pred, _ = dm.predict(Xte, nproc=1)
        acc[solver] = float(np.mean(y_pred == yte))
    print("held-out accuracy", acc)
    assert acc["sklearn"] > 0.5 and abs(acc["device"] - acc["sklearn"]) <= 0.01, acc


# ---- early stopping -------------------------------------------------------------------------------------------------------------------

def test_a_tol_stop_returns_scikit_learns_n_iter(eng):
    """tol = 0.05, n_iter_no_change = 2 on a curve that flattens: every comparison ``loss > best - tol`` the rule makes up to the stop
    is decided by a margin of more than 100 T_loss in the exact run, so rounding cannot move the stop"""
    name = "203x19-17-5-last-batch-11"
    m, F, hidden, k, act, batch, _, shuffle, _, _ = CASES[name]
    R = reference(name)
    Xs = mlp_ref.scale([(R["mean"], R["scale"])], R["D"])
    epochs, tol, nnc = 60, 0.05, 2
    sk64 = sklearn_fit(Xs.astype(np.float64), R["y"], hidden, act, batch, epochs, shuffle, tol=tol, n_iter_no_change=nnc)
    sk32 = sklearn_fit(Xs, R["y"], hidden, act, batch, epochs, shuffle, tol=tol, n_iter_no_change=nnc)
    curve = np.asarray(sk64.loss_curve_)
    best, margin = np.inf, np.inf
    for v in curve:
        if np.isfinite(best):
            margin = min(margin, abs(v - (best - tol)))
        best = min(best, v)
    T_loss = 4 * max(float(np.abs(np.asarray(sk32.loss_curve_) - curve[:len(sk32.loss_curve_)]).max()), U32 * float(curve.max()))
    print(f"tol stop: scikit-learn n_iter_ {sk64.n_iter_} (float32 {sk32.n_iter_}), smallest margin {margin:.3g}, T_loss {T_loss:.3g}")
    assert 3 < sk64.n_iter_ == sk32.n_iter_ < epochs and margin > 100 * T_loss
    res = device_fit(eng, name, max_epochs=epochs, tol=tol, n_iter_no_change=nnc,
                     order=_mlp_fit.schedule(_mlp_fit.layer_sizes(F, hidden, k), act, SEED, m, epochs, shuffle)[2])
    assert res.state == "tol" and res.n_iter == sk64.n_iter_ == len(res.loss_curve)
    assert np.abs(res.loss_curve - curve).max() <= T_loss


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_a_nan_row_ends_the_fit_with_its_state_and_the_context_stays_usable(eng):
    name = "96x16-16-3-whole-tiles"
    m, F, hidden, k, act, batch, epochs, shuffle, _, _ = CASES[name]
    R = reference(name)
    sizes = _mlp_fit.layer_sizes(F, hidden, k)
    W0, B0, order = _mlp_fit.schedule(sizes, act, SEED, m, epochs, shuffle)
    D = np.array(R["D"])
    D[37, 5] = np.nan
    yd = torch.from_numpy(np.array(R["y"])).to(eng.tdev)
    kw = dict(activation=act, n_classes=k, order=order, batch_size=batch, max_epochs=epochs)
    res = eng.mlp_fit(torch.from_numpy(D).to(eng.tdev), yd, W0, B0, mean=R["mean"], scale=R["scale"], **kw)
    assert res.state == "nonfinite_input" and res.n_iter == 0 and len(res.loss_curve) == 0
    for a, b in zip(res.coefs + res.intercepts, W0 + B0):
        assert np.array_equal(a, b)      # nothing was trained
    D[37, 5] = np.inf
    assert eng.mlp_fit(torch.from_numpy(D).to(eng.tdev), yd, W0, B0, **kw).state == "nonfinite_input"
    with pytest.raises(ValueError, match="not finite"):
        models.DTW_MLP.fit(np.random.default_rng(0).normal(size=(m, 8)), R["y"], 3, 0.1, refs=np.zeros((F, 8)), distances=D, scale=False,
                           hidden_layer_sizes=hidden, max_iter=2)
    # a class index the model has no unit for is found on the device, before the first step
    bad_y = np.array(R["y"])
    bad_y[11] = k
    with pytest.raises(ValueError, match="class index"):
        eng.mlp_fit(torch.from_numpy(np.array(R["D"])).to(eng.tdev), torch.from_numpy(bad_y).to(eng.tdev), W0, B0, **kw)
    # the context is usable: the case itself still meets its contract
    f = measure(eng, name)
    assert f["device_err"] <= f["T"], f


def test_a_loss_that_is_not_finite_ends_the_fit_with_its_state_and_the_context_stays_usable(eng):
    """learning_rate_init = 1e38: the first step moves every weight by about 1e38, the second step's products overflow and its loss
    is NaN.  That is arithmetic, not a fault: the fit ends after epoch 1 with WDX_MLP_FIT_NONFINITE_LOSS."""
    from helpers import mlp_fit_rule as rule

    name, epochs, lr = "203x19-17-5-last-batch-11", 3, 1e38
    m, F, hidden, k, act, batch, _, shuffle, _, _ = CASES[name]
    R = reference(name)
    sizes = _mlp_fit.layer_sizes(F, hidden, k)
    W0, B0, order = _mlp_fit.schedule(sizes, act, SEED, m, epochs, shuffle)
    # the float32 rule itself gives a loss that is not finite for epoch 1: otherwise the input is wrong, not the device
    Xs = mlp_ref.scale([(R["mean"], R["scale"])], R["D"])
    for ordered in (True, False):
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            curve = rule.fit(Xs, np.array(R["y"]), k, W0, B0, order, activation=act, batch_size=batch, lr=lr, max_epochs=epochs, ordered=ordered)[2]
        print(f"float32 rule, ordered={ordered}: loss curve {curve}")
        assert not np.isfinite(curve[0]), (ordered, curve)
    res = device_fit(eng, name, max_epochs=epochs, order=order, learning_rate_init=lr)
    print(f"device: state {res.state}, n_iter {res.n_iter}, loss curve {res.loss_curve}")
    assert res.state == "nonfinite_loss" and res.n_iter == 1
    assert res.loss_curve.shape == (1,) and not np.isfinite(res.loss_curve[0])
    with pytest.raises(ValueError, match="the loss of epoch 1 is not finite"):
        models.DTW_MLP.fit(np.random.default_rng(0).normal(size=(m, 8)), R["y"], 3, 0.1, refs=np.zeros((F, 8)), distances=np.array(R["D"]),
                           hidden_layer_sizes=hidden, activation=act, batch_size=batch, max_iter=epochs, random_state=SEED, solver="device",
                           learning_rate_init=lr)
    # the context is usable: an ordinary case still meets its contract
    f = measure(eng, name)
    assert f["state"] == "max_epochs" and f["device_err"] <= f["T"] and f["device_err_loss"] <= f["T_loss"], f


def test_every_refusal_comes_back_before_a_launch(eng):
    m, F, k = 50, 6, 3
    D, y = distances(m, F, k)
    Dd, yd = torch.from_numpy(D).to(eng.tdev), torch.from_numpy(y).to(eng.tdev)

    def fit(hidden=(4,), dist=Dd, yy=yd, classes=k, W=None, B=None, **kw):
        sizes = [F] + list(hidden) + [1 if classes == 2 else classes]
        W0, B0, _ = _mlp_fit.schedule(sizes, "relu", 0, m, 1, False)
        return eng.mlp_fit(dist, yy, W0 if W is None else W, B0 if B is None else B, n_classes=classes, max_epochs=kw.pop("max_epochs", 1), **kw)

    eng.kernel_timing(True)
    try:
        eng.kernel_time_reset()
        for exc, text, kw in [
            (NotImplementedError, "WDX_MLP_FIT_MAX_BATCH", dict(batch_size=_lib.MLP_FIT_MAX_BATCH + 1)),
            (ValueError, "batch_size", dict(batch_size=0)),
            (NotImplementedError, "hidden layers", dict(hidden=(4,) * _lib.MLP_MAX_LAYERS)),
            (NotImplementedError, "WDX_MLP_MAX_WIDTH", dict(hidden=(_lib.MLP_MAX_WIDTH + 1,))),
            (ValueError, "at most 16", dict(classes=17)),
            (ValueError, "at least two", dict(classes=1)),
            (ValueError, "output layer", dict(W=[np.zeros((F, 4), np.float32), np.zeros((4, 2), np.float32)], B=[np.zeros(4, np.float32), np.zeros(2, np.float32)], classes=2)),
            (ValueError, "unknown activation", dict(activation="gelu")),
            (ValueError, "max_iter", dict(max_epochs=0)),
            (ValueError, "n_iter_no_change", dict(n_iter_no_change=-1)),
            (ValueError, "learning_rate_init", dict(learning_rate_init=0.0)),
            (ValueError, "alpha", dict(alpha=-1.0)),
            (ValueError, "beta_1", dict(beta_1=1.0)),
            (ValueError, "epsilon", dict(epsilon=0.0)),
            (ValueError, "tol", dict(tol=float("nan"))),
            (ValueError, "dist must be", dict(dist=Dd.double())),
            (ValueError, "dist must be", dict(dist=Dd.t())),
            (ValueError, "y_idx must be", dict(yy=yd.long())),
            (ValueError, "y_idx must be", dict(yy=yd[:-1])),
            (ValueError, "do not fit the sizes", dict(W=[np.zeros((F + 1, 4), np.float32), np.zeros((4, 3), np.float32)])),
            (ValueError, "mean must hold", dict(mean=np.zeros(F + 1))),
            (ValueError, "order must be", dict(order=np.zeros((2, m), np.int32))),
            (ValueError, "order names a row", dict(order=np.full((1, m), m, np.int32))),
        ]:
            with pytest.raises(exc, match=text):
                fit(**kw)
        # the library's own refusals, past the Python checks: the plan's message comes back as the mapped exception
        sizes = [F, 4, k]
        W0, B0, _ = _mlp_fit.schedule(sizes, "relu", 0, m, 1, False)
        p = _mlp_fit.params_c(sizes, "relu", k, 10, 1, 10, 1e-3, 1e-4, 0.9, 0.999, 1e-8, 1e-4)
        W, B, _, _, _ = _mlp_fit.check_arrays(sizes, m, W0, B0, None, None, None, 1)
        for field, value, exc, text in [("batch_size", _lib.MLP_FIT_MAX_BATCH + 1, NotImplementedError, "WDX_MLP_FIT_MAX_BATCH"),
                                        ("n_classes", 17, NotImplementedError, "more than 16"), ("n_layers", 6, NotImplementedError, "WDX_MLP_MAX_LAYERS"),
                                        ("hidden_activation", 9, ValueError, "unknown hidden activation"), ("lr", -1.0, ValueError, "lr must be")]:
            q = _lib.MlpFitParamsC.from_buffer_copy(p)
            setattr(q, field, value)
            with pytest.raises(exc, match=text):
                _mlp_fit.call(eng.L.wdx_mlp_fit_device, eng.ctx.handle, C.c_void_p(Dd.data_ptr()), m, F, C.c_void_p(yd.data_ptr()), q, W, B, None,
                              None, None, stream=eng._stream())
        with pytest.raises(ValueError, match="ld = 5"):
            _mlp_fit.call(eng.L.wdx_mlp_fit_device, eng.ctx.handle, C.c_void_p(Dd.data_ptr()), m, F - 1, C.c_void_p(yd.data_ptr()), p, W, B, None, None,
                          None, stream=eng._stream())
        ms, launches = eng.kernel_time(_lib.K_MLP_FIT)
        assert launches == 0, launches
    finally:
        eng.kernel_timing(False)
    assert fit().state == "max_epochs"
