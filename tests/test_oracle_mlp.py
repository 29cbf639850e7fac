"""The DTW_MLP tail's restatement (tests/helpers/mlp_ref.py) against scikit-learn on the CPU, and the accuracy contract's
inputs: bitwise float64 path, bitwise scaler steps, dtype rules, the binary [1 - p, p] layout, process_probs, the close-call
cap of the chosen inputs and a positive control that the contract resolves."""
import numpy as np
import pytest

from helpers import mlp_ref

CASES = [  # (n_in, hidden, k, activation, scaler)
    (10, (15,), 3, "relu", None),
    (17, (16,), 2, "logistic", "meanstd"),
    (40, (64, 32), 11, "tanh", "std"),
    (3, (17,), 16, "identity", "meanstd"),
    (101, (100, 50, 25, 12), 11, "relu", None),
]


def _case(i, dtype, n=300, sigma=3.0):
    n_in, hidden, k, act, sc = CASES[i]
    D, _ = mlp_ref.clustered_distances(n, n_in, k, seed=100 + i, sigma=sigma)
    m = mlp_ref.random_mlp(n_in, hidden, k, dtype, act, seed=i)
    return mlp_ref.with_scaler(m, D, sc), D, k


@pytest.mark.parametrize("i", range(len(CASES)))
def test_restatement_is_bitwise_on_the_float64_path(i):
    est, D, _ = _case(i, np.float64)
    got = mlp_ref.sklearn_proba(est, D)
    want = est.predict_proba(D)
    assert got.dtype == want.dtype == np.float64
    assert np.array_equal(got, want)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_restatement_float32_path_close(i):
    est, D, _ = _case(i, np.float32)
    got, want = mlp_ref.sklearn_proba(est, D), est.predict_proba(D)
    assert got.dtype == want.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)


@pytest.mark.parametrize("kind", ["meanstd", "std"])
def test_scaler_steps_bitwise(kind):
    from sklearn.preprocessing import StandardScaler

    D, _ = mlp_ref.clustered_distances(500, 33, 4, seed=7, sigma=5.0)
    s1 = StandardScaler(with_mean=kind == "meanstd").fit(D)
    s2 = StandardScaler().fit(s1.transform(D).astype(np.float64) * 3 + 1)
    steps = [(s.mean_ if s.with_mean else None, s.scale_ if s.with_std else None) for s in (s1, s2)]
    want = s2.transform(s1.transform(D))
    got = mlp_ref.scale(steps, D)
    assert want.dtype == got.dtype == np.float32 and np.array_equal(got, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dtype_rules_and_binary_layout(dtype):
    D, _ = mlp_ref.clustered_distances(200, 12, 2, seed=3)
    m = mlp_ref.random_mlp(12, (9,), 2, dtype, "relu", seed=3)
    assert m.out_activation_ == "logistic" and m.coefs_[-1].shape[1] == 1
    p = m.predict_proba(D)
    assert p.dtype == np.result_type(np.float32, dtype) == dtype
    assert np.array_equal(p[:, 0], (np.asarray(1, dtype) - p[:, 1]).astype(dtype))
    # a float32 model fed float32 distances stays float32; a float64 model runs in float64
    pm = mlp_ref.random_mlp(12, (9,), 5, dtype, "tanh", seed=4).predict_proba(D)
    assert pm.dtype == dtype


def test_process_probs_rules():
    lm = {0: 7, 1: 3, 2: 9}
    p = np.array([[0.4, 0.4, 0.2], [0.1, 0.5, 0.4], [0.3, 0.3, 0.4]], dtype=np.float32)
    pred, conf = mlp_ref.process_probs(p, lm)
    assert pred.tolist() == [7, 3, 9]                      # first maximum on a tie
    assert conf.dtype == np.float32 and conf[0] == 0
    assert conf[1] == np.float32(0.5) - np.float32(0.4)    # margin in the working dtype
    thr = np.array([0.0, float(np.float32(0.5) - np.float32(0.4)), 0.2])
    pred, _ = mlp_ref.process_probs(p, lm, thr)
    assert pred.tolist() == [7, 3, -1]                     # conf < threshold is strict, compared in float64
    thr[1] = np.nextafter(thr[1], 1)
    assert mlp_ref.process_probs(p, lm, thr)[0].tolist() == [7, -1, -1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_close_call_cap_holds_for_the_chosen_inputs(i, dtype):
    est, D, k = _case(i, dtype, n=400 if dtype == np.float64 else 1000)
    thr = np.linspace(0.05, 0.6, k)
    c = mlp_ref.contract(est, D, thr)
    print(f"case {i} {np.dtype(dtype).name}: E_ref {c['e_ref']:.3g} T {c['T']:.3g} close {int(c['close'].sum())}")
    assert c["close"].mean() <= 0.01
    if dtype == np.float64:
        assert c["e_ref"] < 1e-13
    else:
        assert c["e_ref"] < 1e-4


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_positive_control_resolves_on_cpu(dtype):
    est, D, k = _case(0, dtype)
    c = mlp_ref.contract(est, D, None)
    e2, moved = mlp_ref.perturb_first_layer(est, D, c["T"])
    p2 = mlp_ref.exact_proba(e2, D).astype(np.float64)
    pred2, conf2 = mlp_ref.process_probs(p2, {i: i for i in range(k)})
    pred_sk, _ = mlp_ref.process_probs(c["p_sk"], {i: i for i in range(k)})
    _, bad = mlp_ref.check_outputs(c, p2, conf2, pred2, pred_sk, np.float64)
    assert moved >= 10 * c["T"] and bad
    # ... while the unperturbed exact outputs pass
    p1 = c["p_ex"].astype(np.float64)
    pred1, conf1 = mlp_ref.process_probs(p1, {i: i for i in range(k)})
    _, ok = mlp_ref.check_outputs(c, p1, conf1, pred1, pred_sk, np.float64)
    assert not ok, ok
