"""The classifier tail of DTW_SVM.predict restated in NumPy float64, vectorised over reads (test infrastructure).

libsvm's svm_predict_probability for a precomputed kernel (svm.cpp: svm_predict_values, sigmoid_predict,
multiclass_probability) followed by process_probs (models/utils.py:45-61), in libsvm's operation order: the
decision sums are sequential loops over the support vectors, Qp and pQp sequential over the classes.  Pinned to the
oracle's C restatement in tests/test_oracle_svm.py.

Besides the outputs it reports, per read, the coupling's STOPPING MARGIN: the minimum over the executed iterations of
|max_error - eps| / eps.  Two implementations that agree to rounding can still stop one sweep apart when max_error
lands within rounding of eps (probabilities then move by up to ~1e-3); tight comparisons skip reads whose margin is
below a stated bound.

``synth_model`` makes libsvm parameter sets without training (models from seeds, no fixtures).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

MIN_PROB = 1e-7

# (pwr_dist, gamma, far distance v): gamma * v^p >= 110, so exp(-gamma v^p) is exactly 0 in float32, while what a wrong
# kernel would use -- gamma * v^(p-1) (power off by one, p >= 2) or v (gamma dropped, p = 1) -- stays <= 16, so such a
# kernel gives K >= 1e-7
EXACT_KERNELS = [(1, 8.0, 14.0), (2, 2.0, 8.0), (3, 0.25, 8.0), (1, 7.5, 15.0), (2, 0.5, 15.0)]

N_SUPPORT_CYCLE = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129]


@dataclass
class SvmRef:
    prob: np.ndarray        # (n, k)
    dec: np.ndarray         # (n, npairs) one-vs-one decision values
    fApB: np.ndarray        # (n, npairs) dec * probA + probB
    sigmoid: np.ndarray     # (n, npairs) Platt sigmoid before the [1e-7, 1 - 1e-7] clip
    margin: np.ndarray      # (n,) stopping margin of the coupling
    iters: np.ndarray       # (n,) executed coupling iterations (checks of max_error)
    pred: np.ndarray        # (n,) label, -1 under the threshold
    conf: np.ndarray        # (n,) top1 - top2


def _pairs(k):
    return [(i, j) for i in range(k) for j in range(i + 1, k)]


def predict(K, n_support, support, dual_coef, rho, probA, probB, label_map=None, thresholds=None) -> SvmRef:
    """K: (n, n_train) kernel rows (any float dtype, widened to float64)."""
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    n_support = np.asarray(n_support, dtype=np.int64)
    k = n_support.size
    start = np.concatenate([[0], np.cumsum(n_support)])
    kv = K[:, np.asarray(support, dtype=np.int64)]
    pairs = _pairs(k)
    npairs = len(pairs)
    dec = np.empty((n, npairs))
    for p, (i, j) in enumerate(pairs):
        s = np.zeros(n)
        si, sj = start[i], start[j]
        c1, c2 = dual_coef[j - 1], dual_coef[i]
        for q in range(n_support[i]):
            s = s + c1[si + q] * kv[:, si + q]
        for q in range(n_support[j]):
            s = s + c2[sj + q] * kv[:, sj + q]
        dec[:, p] = s - rho[p]
    fApB = dec * np.asarray(probA)[None, :] + np.asarray(probB)[None, :]
    with np.errstate(over="ignore"):
        e_neg, e_pos = np.exp(-fApB), np.exp(fApB)
        sig = np.where(fApB >= 0, e_neg / (1.0 + e_neg), 1.0 / (1.0 + e_pos))
    v = np.minimum(np.maximum(sig, MIN_PROB), 1 - MIN_PROB)
    r = np.empty((n, k, k))
    for p, (i, j) in enumerate(pairs):
        r[:, i, j] = v[:, p]
        r[:, j, i] = 1 - v[:, p]
    prob, margin, iters = _multiclass_probability(r)
    best = np.argmax(prob, axis=1)
    srt = np.sort(prob, axis=1)
    conf = srt[:, -1] - srt[:, -2]
    lab = np.arange(k) if label_map is None else np.asarray(label_map)
    pred = lab[best].astype(np.int64)
    if thresholds is not None:
        pred[conf < np.asarray(thresholds)[best]] = -1
    return SvmRef(prob, dec, fApB, sig, margin, iters, pred, conf)


def _multiclass_probability(r):
    n, k, _ = r.shape
    Q = np.zeros((n, k, k))
    for t in range(k):
        for j in range(k):
            if j != t:
                Q[:, t, t] += r[:, j, t] * r[:, j, t]
        for j in range(k):
            if j != t:
                Q[:, t, j] = -r[:, j, t] * r[:, t, j]
    p = np.full((n, k), 1.0 / k)
    eps = 0.005 / k
    max_iter = max(100, k)
    live = np.ones(n, dtype=bool)
    margin = np.full(n, np.inf)
    iters = np.zeros(n, dtype=np.int64)
    Qp = np.zeros((n, k))
    for _ in range(max_iter):
        Qp_new = np.zeros((n, k))
        for j in range(k):
            Qp_new = Qp_new + Q[:, :, j] * p[:, j:j + 1]
        pQp = np.zeros(n)
        for t in range(k):
            pQp = pQp + p[:, t] * Qp_new[:, t]
        err = np.abs(Qp_new - pQp[:, None]).max(axis=1)
        Qp = np.where(live[:, None], Qp_new, Qp)
        margin = np.where(live, np.minimum(margin, np.abs(err - eps) / eps), margin)
        iters += live
        live &= ~(err < eps)
        if not live.any():
            break
        pn, qn, pqn = p.copy(), Qp.copy(), pQp.copy()
        for t in range(k):
            Qtt = Q[:, t, t]
            diff = (-qn[:, t] + pqn) / Qtt
            pn[:, t] += diff
            pqn = (pqn + diff * (diff * Qtt + 2 * qn[:, t])) / (1 + diff) / (1 + diff)
            qn = (qn + diff[:, None] * Q[:, t, :]) / (1 + diff)[:, None]
            pn = pn / (1 + diff)[:, None]
        p = np.where(live[:, None], pn, p)
        Qp = np.where(live[:, None], qn, Qp)
    return p, margin, iters


@dataclass
class SynthModel:
    k: int
    n_train: int
    n_support: np.ndarray
    support: np.ndarray
    dual_coef: np.ndarray
    rho: np.ndarray
    probA: np.ndarray
    probB: np.ndarray
    label_map: np.ndarray
    thresholds: Optional[np.ndarray]
    gamma: float
    pwr_dist: int

    def arrays(self):
        """the positional arrays of orc.svm_predict_proba / predict"""
        return self.n_support, self.support, self.dual_coef, self.rho, self.probA, self.probB

    def to_dtw_svm(self, X_train, window=15, penalty=0.1):
        from warpdemux_amd.models import DTW_SVM

        return DTW_SVM(X_train, self.n_support, self.support, self.dual_coef, self.rho, self.probA, self.probB,
                       {i: int(self.label_map[i]) for i in range(self.k)}, self.thresholds, window=window, penalty=penalty,
                       gamma=self.gamma, pwr_dist=self.pwr_dist, block_size=1000)

    def predict(self, K):
        return predict(K, *self.arrays(), label_map=self.label_map, thresholds=self.thresholds)


def synth_model(k, seed, n_support=None, n_extra=40, thresholds=True, gamma=1.0, pwr_dist=1) -> SynthModel:
    """libsvm parameters without training: distinct unsorted support indices, dual_coef ~ N(0, 1) with some exact zeros,
    random rho, probA = -U(0.3, 4), probB ~ N(0, 0.5), a non-identity label map, thresholds U(0.05, 0.6) or None.
    ``n_support`` defaults to N_SUPPORT_CYCLE read from position ``seed``."""
    rng = np.random.default_rng(seed)
    if n_support is None:
        n_support = [N_SUPPORT_CYCLE[(seed + c) % len(N_SUPPORT_CYCLE)] for c in range(k)]
    n_support = np.ascontiguousarray(n_support, dtype=np.int32)
    n_sv = int(n_support.sum())
    n_train = n_sv + n_extra
    support = rng.permutation(n_train)[:n_sv].astype(np.int32)
    dual_coef = rng.normal(size=(k - 1, n_sv))
    dual_coef[rng.random(dual_coef.shape) < 0.05] = 0.0
    npairs = k * (k - 1) // 2
    rho = rng.normal(0, 1.0, npairs)
    probA = -rng.uniform(0.3, 4.0, npairs)
    probB = rng.normal(0, 0.5, npairs)
    label_map = (rng.permutation(k) * 3 + 1).astype(np.int32)
    thr = rng.uniform(0.05, 0.6, k) if thresholds else None
    return SynthModel(k, n_train, n_support, support, np.ascontiguousarray(dual_coef), rho, probA, probB, label_map, thr,
                      float(gamma), int(pwr_dist))


def exact_distances(n, n_train, far, seed, inf_share=0.15, big_share=0.15):
    """(n, n_train) float32 distances: 0 at a density drawn per read from U(0.02, 0.30), the rest ``far``, 1e4 or +inf."""
    rng = np.random.default_rng(seed)
    dens = rng.uniform(0.02, 0.30, n)
    D = np.full((n, n_train), np.float32(far), dtype=np.float32)
    u = rng.random((n, n_train))
    D[u < inf_share] = np.inf
    D[(u >= inf_share) & (u < inf_share + big_share)] = np.float32(1e4)
    D[rng.random((n, n_train)) < dens[:, None]] = 0.0
    return D
