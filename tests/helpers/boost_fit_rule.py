"""The Fpt_Boost trainer restated in NumPy: the defining document of wdx_boost_fit.hip (include/wdx.h: wdx_boost_fit_device states the
same rule).  Everything here is written from the rule, not from the library's Python: the borders, the bins, exp_rule,
the quantised gradients, the integer histograms, the float64 score in its stated order, the first-maximum split, the leaf values
and the score update.  Integer sums are exact in any order and every float64 expression below has the stated operation order, so
the device's splits, leaves and scores are held to these with ``np.array_equal``.
"""
from __future__ import annotations

import numpy as np

from . import boost_ref

GRAD_BITS = 20
LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42feep-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
EXP_DEGREE = 13
EXP_COEF = [1.0]
for _i in range(1, EXP_DEGREE + 1):
    EXP_COEF.append(EXP_COEF[-1] / float(_i))     # c_i = c_{i-1} / i


class Refused(ValueError):
    """the rule refuses the fit (no feature has a border)"""


def exp_rule(x):
    """exp(x) for float64 x <= 0, elementwise: 0 below -700; else k = rint(x log2e), r = (x - k LN2_HI) - k LN2_LO, a degree-13 Horner
    polynomial with separate multiply and add, ldexp(P, k)."""
    x = np.asarray(x, dtype=np.float64)
    below = x < -700.0
    x = np.where(below, 0.0, x)              # (those come out 0: nothing is computed of them)
    k = np.rint(x * LOG2E)
    r = (x - k * LN2_HI) - k * LN2_LO
    P = np.full(x.shape, EXP_COEF[EXP_DEGREE])
    for i in range(EXP_DEGREE - 1, -1, -1):
        P = P * r
        P = P + EXP_COEF[i]
    return np.where(below, 0.0, np.ldexp(P, k.astype(np.int32)))


def feature_borders(col32, B):
    col32 = np.asarray(col32, dtype=np.float32)
    s = np.sort(col32[~np.isnan(col32)])
    u = np.unique(s)
    if len(u) <= 1:
        return np.zeros(0, np.float32)
    if len(u) - 1 <= B:
        return u[:-1]
    m = len(s)
    picks = np.array([s[(j * m) // (B + 1)] for j in range(1, B + 1)], dtype=np.float32)
    b = np.unique(picks)
    return b[b != u[-1]]


def to_f32(X):
    with np.errstate(over="ignore"):
        return np.asarray(X, dtype=np.float64).astype(np.float32)


def borders(X, B):
    X32 = to_f32(X)
    return [feature_borders(X32[:, f], B) for f in range(X32.shape[1])]


def binarise(X, border_list):
    """(F, n) uint8: the number of the feature's borders with x > border in float32; NaN gives 0."""
    X32 = to_f32(X)
    bins = np.zeros((X32.shape[1], X32.shape[0]), dtype=np.uint8)
    for f, b in enumerate(border_list):
        with np.errstate(invalid="ignore"):
            bins[f] = (X32[:, f][:, None] > np.asarray(b, dtype=np.float32)[None, :]).sum(axis=1)
    return bins


def gradients(S, y):
    """(n, k) int64 quantised gradients of the scores S (n, k) float64 and the class indices y."""
    S = np.asarray(S, dtype=np.float64)
    n, k = S.shape
    z = S - S.max(axis=1)[:, None]
    e = exp_rule(z)
    tot = np.zeros(n)
    for c in range(k):                       # class order
        tot = tot + e[:, c]
    p = e / tot[:, None]
    g = (np.asarray(y)[:, None] == np.arange(k)[None, :]).astype(np.float64) - p
    return np.rint(g * float(1 << GRAD_BITS)).astype(np.int64)


def one_tree(bins, border_list, q, depth, lam, lr):
    """(features int32[depth], border indices int32[depth], leaves float64 (2**depth, k), leaf index int64[n]) of one tree."""
    F, n = bins.shape
    k = q.shape[1]
    active = [f for f in range(F) if len(border_list[f]) > 0]
    if not active:
        raise Refused("no feature has a border")
    nb = np.array([len(b) for b in border_list])
    NB = int(nb.max()) + 1                   # bins per feature, padded: a bin beyond a feature's own stays empty
    valid = np.arange(NB - 1)[None, :] < nb[:, None]            # (F, NB - 1): border b exists in feature f
    bins64 = bins.astype(np.int64)
    leaf = np.zeros(n, dtype=np.int64)
    feats, bidx = [], []
    for level in range(depth):
        L = 1 << level
        # integer histograms per (feature, leaf, bin): the count and the k gradient sums.  (bincount adds float64 weights: every
        # partial sum is an integer below 2^53, so the sums are exact in any order, as the device's integer atomics are.)
        cell = ((np.arange(F)[:, None] * L + leaf[None, :]) * NB + bins64).reshape(-1)
        N = np.bincount(cell, minlength=F * L * NB).reshape(F, L, NB)
        NLc = np.cumsum(N, axis=2)
        acc = np.zeros((F, NB - 1))
        GLc = []
        for c in range(k):
            G = np.bincount(cell, weights=np.tile(q[:, c].astype(np.float64), F), minlength=F * L * NB).astype(np.int64).reshape(F, L, NB)
            GLc.append(np.cumsum(G, axis=2))
        for lf in range(L):                  # leaf ascending, class ascending: the left term, then the right term
            NL = NLc[:, lf, :-1].astype(np.float64)
            NR = (NLc[:, lf, -1:] - NLc[:, lf, :-1]).astype(np.float64)
            for c in range(k):
                GL = GLc[c][:, lf, :-1].astype(np.float64)
                GR = (GLc[c][:, lf, -1:] - GLc[c][:, lf, :-1]).astype(np.float64)
                acc = acc + GL * GL / (NL + lam)
                acc = acc + GR * GR / (NR + lam)
        flat = np.where(valid, acc, -np.inf).reshape(-1)
        at = int(np.argmax(flat))            # the first maximum in (f, b) order: the lowest f, then the lowest b among equals
        f, b = divmod(at, NB - 1)
        feats.append(f), bidx.append(b)
        leaf |= (bins64[f] > b).astype(np.int64) << level
    leaves = np.zeros((1 << depth, k))
    Nl = np.bincount(leaf, minlength=1 << depth).astype(np.float64)
    inv = 1.0 / float(1 << GRAD_BITS)
    for c in range(k):
        Gl = np.bincount(leaf, weights=q[:, c].astype(np.float64), minlength=1 << depth).astype(np.int64)
        leaves[:, c] = lr * ((Gl.astype(np.float64) * inv) / (Nl + lam))
    return np.array(feats, np.int32), np.array(bidx, np.int32), leaves, leaf


class Fit:
    def __init__(self, border_list, k):
        self.borders, self.k = border_list, k
        self.split_feature, self.split_border, self.leaf_values = [], [], []

    def trees(self):
        """(features, float32 border values, leaves) per tree -- boost_ref.BoostModel's form"""
        return [(f, np.array([self.borders[ff][bb] for ff, bb in zip(f, b)], dtype=np.float32), lv)
                for f, b, lv in zip(self.split_feature, self.split_border, self.leaf_values)]

    def model(self, n_features):
        return boost_ref.BoostModel(self.trees(), n_features, self.k, 1.0, np.zeros(self.k))


def fit(X, y, k, n_trees, depth, lr, lam, B, scores=None, border_list=None):
    """(Fit, scores): n_trees more trees from ``scores`` (None: zeros), which is not modified."""
    X = np.asarray(X, dtype=np.float64)
    border_list = borders(X, B) if border_list is None else border_list
    bins = binarise(X, border_list)
    S = np.zeros((len(X), k)) if scores is None else np.array(scores, dtype=np.float64)
    out = Fit(border_list, k)
    for _ in range(n_trees):
        q = gradients(S, y)
        f, b, leaves, leaf = one_tree(bins, border_list, q, depth, float(lam), float(lr))
        out.split_feature.append(f), out.split_border.append(b), out.leaf_values.append(leaves)
        S = S + leaves[leaf]
    return out, S


def logloss(S, y):
    S = np.asarray(S, dtype=np.float64)
    z = S - S.max(axis=1)[:, None]
    return float(np.mean(np.log(np.exp(z).sum(axis=1)) - z[np.arange(len(z)), np.asarray(y)]))


def synthetic(n, F, k, seed, noise=1.5):
    """templates plus N(0, noise) noise: (X float64 (n, F), y int64 (n,))"""
    rng = np.random.default_rng(seed)
    templates = rng.normal(0, 2.0, (k, F))
    y = rng.integers(0, k, n)
    return templates[y] + rng.normal(0, noise, (n, F)), y
