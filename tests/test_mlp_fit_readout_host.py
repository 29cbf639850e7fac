"""What the accuracy cases of tests/test_gpu_mlp_fit.py can and cannot see, measured without a GPU on the float32 restatement of the
trainer's rule (tests/helpers/mlp_fit_rule.py, every product accumulated strictly in k order) under that file's own contract:
T = 4 max(E_ref, u max|theta|) around scikit-learn's float64 run, E_ref = max |scikit-learn float32 - float64|.

The gradient product of W_1 (A_1^T delta_2, 17 x nb times nb x 33) is made wrong in one of two ways:
  scaled    the tile [16:, 32:] is 1.0001 times too large (a wrong divisor, a mis-scaled term, a moment carried with the wrong weight)
  dropped   the last batch row's term is missing on columns 16 and up (a chain that ends one row early)
Adam with epsilon = 1e-8 normalises the gradient, so under scikit-learn's default hyper-parameters `scaled` stays inside T: that blind
spot is asserted here, so that the read-out cases (RO: beta_1 = beta_2 = 0, epsilon = 1, learning_rate_init = 1, the update
-g / (|g| + 1)) are not taken for redundant.  Under RO both mutations exceed T.

The last test is the reference's own check: unmutated, the restatement meets T and T_loss on every case the GPU test adds, so a device
failure there is a finding about the kernels and not about the contract."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import test_gpu_mlp_fit as gpu  # noqa: E402  (its cases, its hyper-parameters and its scikit-learn references; nothing of it needs a GPU here)
from helpers import mlp_fit_rule as rule  # noqa: E402
from helpers import mlp_ref  # noqa: E402

RULE_NAMES = dict(learning_rate_init="lr", beta_1="beta1", beta_2="beta2")
# the cases this file's last test holds the restatement to: everything the GPU test runs beyond scikit-learn's defaults at small shapes
NEW_CASES = [n for n in gpu.CASES if n in gpu.HYPER or n.startswith(("max-depth", "width-", "tiny-", "batch-1024"))]

READOUT = gpu.CASES["readout-tanh"]          # 37 x 19 -> 17 -> 33 -> 5, one step of 37 rows, one epoch
MUTATIONS = ("scaled", "dropped")


def restate(spec, hyper, R):
    """(flat parameters, loss curve) of the float32 restatement, ordered, on the case's scaled input"""
    m, F, hidden, k, act, batch, epochs, shuffle, _, _ = spec
    Xs = mlp_ref.scale([(R["mean"], R["scale"])], R["D"])
    sizes = [F] + list(hidden) + [1 if k == 2 else k]
    W0, B0, order = rule.init_and_order(sizes, act, gpu.SEED, m, epochs, shuffle, dtype=np.float32)
    kw = {RULE_NAMES.get(key, key): v for key, v in dict(hyper).items()}
    W, B, curve, stopped = rule.fit(Xs, np.array(R["y"]), k, W0, B0, order, activation=act, batch_size=batch, max_epochs=epochs, ordered=True, **kw)
    assert all(a.dtype == np.float32 for a in W + B) and not stopped and len(curve) == epochs == R["n_iter"]
    return gpu._flat(W, B), curve


def figures(spec, hyper, mutation=None, monkeypatch=None):
    """(error / T of the parameters, error / T_loss of the loss curve) of the restatement, with the W_1 gradient product mutated"""
    R = gpu.reference_of(spec, tuple(sorted(dict(hyper).items())))
    if mutation is not None:
        plain, hits = rule._matmul, []

        def wrong(a, b, ordered):
            out = plain(a, b, ordered)
            if a.shape[0] == 17 and b.shape[1] == 33 and a.shape[1] == b.shape[0] and a.shape[1] != 17:
                hits.append(a.shape[1])
                if mutation == "scaled":
                    out[16:, 32:] *= np.float32(1.0001)
                else:
                    out[:, 16:] = plain(a[:, :-1], b[:-1, 16:], ordered)
            return out

        monkeypatch.setattr(rule, "_matmul", wrong)
        th, curve = restate(spec, hyper, R)
        monkeypatch.setattr(rule, "_matmul", plain)
        steps = -(-spec[0] // min(spec[5], spec[0])) * spec[6]
        assert len(hits) == steps, (hits, steps)    # the mutation met the product it names, once per step
    else:
        th, curve = restate(spec, hyper, R)
    return float(np.abs(th - R["th64"]).max()) / R["T"], float(np.abs(curve - R["l64"]).max()) / R["T_loss"]


def test_read_out_sees_both_mutations(monkeypatch):
    base = figures(READOUT, gpu.RO)[0]
    got = {mu: figures(READOUT, gpu.RO, mu, monkeypatch)[0] for mu in MUTATIONS}
    print(f"read-out, error / T: unmutated {base:.3g}, scaled {got['scaled']:.3g}, dropped {got['dropped']:.3g}")
    assert base <= 1 < got["scaled"] and got["dropped"] > 1, (base, got)


def test_default_hyper_parameters_do_not_see_a_scaled_gradient(monkeypatch):
    """the blind spot: one step at scikit-learn's defaults moves every weight by lr sign(g) whatever |g| is"""
    base = figures(READOUT, {})[0]
    got = {mu: figures(READOUT, {}, mu, monkeypatch)[0] for mu in MUTATIONS}
    print(f"defaults, error / T: unmutated {base:.3g}, scaled {got['scaled']:.3g}, dropped {got['dropped']:.3g}")
    assert base <= 1 and got["scaled"] <= 1 < got["dropped"], (base, got)


@pytest.mark.parametrize("name", NEW_CASES)
def test_the_restatement_meets_the_contract_on_every_new_case(name):
    r, r_loss = figures(gpu.CASES[name], gpu.HYPER.get(name, {}))
    print(f"{name}: error / T {r:.3g}, loss error / T_loss {r_loss:.3g}")
    assert r <= 1 and r_loss <= 1, (name, r, r_loss)
