"""NumPy restatement of the trainer behind DTW_MLP.fit (include/wdx.h: wdx_mlp_fit_device states the rule): scikit-learn's
``MLPClassifier(solver="adam")`` on an already scaled input, with the random draws made explicit.

It works in the dtype of its input -- float64 (equal to scikit-learn to rounding of the last bit: tests/test_mlp_fit_rule_host.py) or
float32 (the device trainer's arithmetic; ``ordered=True`` accumulates every matrix product strictly in k order, as the MFMA chains do).
Nothing here imports the package: the package's own schedule (`warpdemux_amd._mlp_fit`) is compared with this one."""
import numpy as np
from scipy.special import expit, xlogy


def init_and_order(sizes, activation, seed, m, max_epochs, shuffle=True, dtype=np.float64):
    """(coefs, intercepts, order): scikit-learn's draws from ONE ``RandomState(seed)`` -- per layer ``uniform(-b, b, (fan_in, fan_out))``
    then ``uniform(-b, b, fan_out)``, ``b = sqrt(6 / (fan_in + fan_out))`` (2 for logistic hidden units); then per epoch a permutation
    of ``arange(m)`` applied to the order so far.  ``order`` is (max_epochs, m) int32, or None without shuffling."""
    rs = np.random.RandomState(seed)
    factor = 2.0 if activation == "logistic" else 6.0
    coefs, intercepts = [], []
    for fi, fo in zip(sizes[:-1], sizes[1:]):
        b = np.sqrt(factor / (fi + fo))
        coefs.append(rs.uniform(-b, b, (fi, fo)).astype(dtype))
        intercepts.append(rs.uniform(-b, b, fo).astype(dtype))
    order = None
    if shuffle:
        order = np.empty((max_epochs, m), np.int32)
        idx = np.arange(m)
        for e in range(max_epochs):
            perm = np.arange(m)
            rs.shuffle(perm)
            idx = idx[perm]
            order[e] = idx
    return coefs, intercepts, order


def stop_epoch(loss_curve, tol, n_iter_no_change):
    """Index of the last epoch scikit-learn runs on this loss curve (its ``n_iter_`` - 1), and whether ``tol`` stopped it."""
    best, count = np.inf, 0
    for e, loss in enumerate(loss_curve):
        count = count + 1 if loss > best - tol else 0
        if loss < best:
            best = loss
        if count > n_iter_no_change:
            return e, True
    return len(loss_curve) - 1, False


def _act(z, activation):
    if activation == "relu":
        return np.maximum(z, 0)
    if activation == "tanh":
        return np.tanh(z)
    if activation == "logistic":
        return expit(z)
    return z


def _dact(a, d, activation):
    if activation == "relu":
        d[a == 0] = 0
    elif activation == "tanh":
        d *= 1 - a ** 2
    elif activation == "logistic":
        d *= a
        d *= 1 - a
    return d


def _matmul(a, b, ordered):
    if not ordered:
        return a @ b
    acc = np.zeros((a.shape[0], b.shape[1]), a.dtype)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * b[k]
    return acc


def fit(Xs, y_idx, n_classes, coefs, intercepts, order, activation="relu", alpha=1e-4, batch_size=200, lr=1e-3, beta1=0.9,
        beta2=0.999, epsilon=1e-8, max_epochs=200, tol=1e-4, n_iter_no_change=10, ordered=False):
    """(coefs, intercepts, loss_curve, stopped_by_tol) after training on the scaled input ``Xs`` (m, F) in its own dtype."""
    dt = Xs.dtype
    m = Xs.shape[0]
    W = [np.array(c, dtype=dt) for c in coefs]
    B = [np.array(b, dtype=dt) for b in intercepts]
    nl = len(W)
    n_out = W[-1].shape[1]
    Y = (y_idx == 1).astype(dt)[:, None] if n_out == 1 else np.eye(n_classes, dtype=dt)[y_idx]
    params = W + B
    ms = [np.zeros_like(p) for p in params]
    vs = [np.zeros_like(p) for p in params]
    bs = int(np.clip(batch_size, 1, m))
    eps = np.finfo(dt).eps
    t, curve, best, count, stopped = 0, [], np.inf, 0, False
    for epoch in range(max_epochs):
        idx = np.arange(m) if order is None else order[epoch]
        acc_loss = 0.0
        for b0 in range(0, m, bs):
            rows = idx[b0:b0 + bs]
            nb = len(rows)
            A = [Xs[rows]]
            for l in range(nl):
                z = _matmul(A[l], W[l], ordered)
                z += B[l]
                A.append(_act(z, activation) if l < nl - 1 else z)
            z = A[-1]
            if n_out == 1:
                p = expit(z)
            else:
                e = np.exp(z - z.max(axis=1)[:, None])
                p = e / e.sum(axis=1)[:, None]
            pc = np.clip(p, eps, 1 - eps)
            if n_out == 1:
                ce = -np.average(xlogy(Y[rows], pc) + xlogy(1 - Y[rows], 1 - pc), axis=0).sum()
            else:
                ce = -np.average(xlogy(Y[rows], pc), axis=0).sum()
            values = 0
            for w in W:
                values += np.dot(w.ravel(), w.ravel())
            acc_loss += (ce + (0.5 * alpha) * values / nb) * nb
            delta = p - Y[rows]
            gW, gB = [None] * nl, [None] * nl
            for l in range(nl - 1, -1, -1):
                g = _matmul(A[l].T, delta, ordered)
                g += alpha * W[l]
                g /= nb
                gW[l], gB[l] = g, np.sum(delta, axis=0) / nb
                if l > 0:
                    delta = _dact(A[l], _matmul(delta, W[l].T, ordered), activation)
            t += 1
            grads = gW + gB
            lr_t = lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
            for i, (p_, g) in enumerate(zip(params, grads)):
                ms[i] = beta1 * ms[i] + (1 - beta1) * g
                vs[i] = beta2 * vs[i] + (1 - beta2) * (g ** 2)
                p_ += -lr_t * ms[i] / (np.sqrt(vs[i]) + epsilon)
        curve.append(acc_loss / m)
        count = count + 1 if curve[-1] > best - tol else 0
        if curve[-1] < best:
            best = curve[-1]
        if count > n_iter_no_change:
            stopped = True
            break
    return W, B, np.array(curve, dtype=np.float64), stopped
