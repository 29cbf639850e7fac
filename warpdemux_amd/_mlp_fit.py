"""Host code around the device MLP trainer (include/wdx.h: wdx_mlp_fit_device states the trainer's rule): scikit-learn's random
draws, its stop rule, and the call.

With an integer ``random_state``, ``MLPClassifier(solver="adam")`` draws its initial weights and then every epoch's shuffle from ONE
``np.random.RandomState(seed)``: per layer ``uniform(-b, b, (fan_in, fan_out))`` and ``uniform(-b, b, fan_out)`` with
``b = sqrt(6 / (fan_in + fan_out))`` (2 instead of 6 for logistic hidden units), then per epoch ``perm = arange(m); rs.shuffle(perm)``
applied to the order so far (``idx = idx[perm]``).  `schedule` makes exactly those draws, so the device trainer follows scikit-learn's
own trajectory with rounding as the only difference (tests/helpers/mlp_fit_rule.py restates the whole rule in NumPy)."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _lib

ACTIVATIONS = ("identity", "logistic", "tanh", "relu")


class FitResult(NamedTuple):
    coefs: list          # float32 (fan_in, fan_out) per layer
    intercepts: list     # float32 (fan_out,) per layer
    loss_curve: np.ndarray   # float64, one value per epoch run
    n_iter: int
    state: str           # one of _lib.MLP_FIT_STATES


def layer_sizes(n_in: int, hidden_layer_sizes, n_classes: int):
    """[n_in, hidden..., n_out]: n_out = n_classes, or one logistic unit for two classes.  ValueError / NotImplementedError as the
    library would refuse them."""
    hidden = [hidden_layer_sizes] if np.isscalar(hidden_layer_sizes) else list(hidden_layer_sizes)
    if not hidden or any(not isinstance(h, (int, np.integer)) or h < 1 for h in hidden):
        raise ValueError(f"hidden_layer_sizes must be one or more positive integers, not {hidden_layer_sizes!r}")
    if len(hidden) + 1 > _lib.MLP_MAX_LAYERS:
        raise NotImplementedError(f"{len(hidden)} hidden layers: the resident MLP tail serves at most {_lib.MLP_MAX_LAYERS - 1}")
    if max(hidden) > _lib.MLP_MAX_WIDTH:
        raise NotImplementedError(f"a hidden layer of {max(hidden)} units: the resident MLP tail serves at most {_lib.MLP_MAX_WIDTH}")
    return [int(n_in)] + [int(h) for h in hidden] + [1 if n_classes == 2 else int(n_classes)]


def check_seed(random_state):
    if not isinstance(random_state, (int, np.integer)) or isinstance(random_state, bool) or random_state < 0:
        raise ValueError(f'solver="device" needs a non-negative integer random_state, not {random_state!r}')
    return int(random_state)


def schedule(sizes: Sequence[int], activation: str, seed: int, m: int, max_epochs: int, shuffle: bool = True):
    """(coefs, intercepts, order): float32 initial weights and the (max_epochs, m) int32 order table (None without shuffling), drawn
    as scikit-learn draws them (module docstring)."""
    rs = np.random.RandomState(check_seed(seed))
    factor = 2.0 if activation == "logistic" else 6.0
    coefs, intercepts = [], []
    for fan_in, fan_out in zip(sizes[:-1], sizes[1:]):
        bound = np.sqrt(factor / (fan_in + fan_out))
        coefs.append(rs.uniform(-bound, bound, (fan_in, fan_out)).astype(np.float32))
        intercepts.append(rs.uniform(-bound, bound, fan_out).astype(np.float32))
    if not shuffle:
        return coefs, intercepts, None
    order = np.empty((max_epochs, m), np.int32)
    idx = np.arange(m)
    for e in range(max_epochs):
        perm = np.arange(m)
        rs.shuffle(perm)
        idx = idx[perm]
        order[e] = idx
    return coefs, intercepts, order


def stop_epoch(loss_curve, tol: float, n_iter_no_change: int):
    """(index of the last epoch scikit-learn would run on this loss curve, whether ``tol`` ended it): after each epoch
    ``count = count + 1 if loss > best - tol else 0``, ``best = min(best, loss)``, stop when ``count > n_iter_no_change``."""
    best, count = np.inf, 0
    for e, loss in enumerate(loss_curve):
        count = count + 1 if loss > best - tol else 0
        best = min(best, loss)
        if count > n_iter_no_change:
            return e, True
    return len(loss_curve) - 1, False


def params_c(sizes, activation, n_classes, batch_size, max_epochs, n_iter_no_change, lr, alpha, beta1, beta2, epsilon, tol):
    """wdx_mlp_fit_params of one fit; what Python can name of the plan's refusals is raised here, before any device work."""
    if activation not in ACTIVATIONS:
        raise ValueError(f"unknown activation {activation!r}: one of {ACTIVATIONS}")
    if n_classes < 2:
        raise ValueError(f"fit needs at least two classes, found {n_classes}")
    if n_classes > _lib.MLP_FIT_MAX_CLASSES:
        raise ValueError(f"{n_classes} classes: the resident MLP tail serves at most {_lib.MLP_FIT_MAX_CLASSES}")
    if len(sizes) - 1 > _lib.MLP_MAX_LAYERS or len(sizes) < 3:
        raise NotImplementedError(f"{len(sizes) - 2} hidden layers: 1 .. {_lib.MLP_MAX_LAYERS - 1} are served")
    if not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f"batch_size must be a positive integer, not {batch_size!r}")
    if batch_size > _lib.MLP_FIT_MAX_BATCH:
        raise NotImplementedError(f"batch_size = {batch_size}, more than WDX_MLP_FIT_MAX_BATCH = {_lib.MLP_FIT_MAX_BATCH}")
    if not isinstance(max_epochs, (int, np.integer)) or max_epochs < 1:
        raise ValueError(f"max_iter must be a positive integer, not {max_epochs!r}")
    if not isinstance(n_iter_no_change, (int, np.integer)) or n_iter_no_change < 0:
        raise ValueError(f"n_iter_no_change must be a non-negative integer, not {n_iter_no_change!r}")
    for name, v in (("learning_rate_init", lr), ("epsilon", epsilon)):
        if not (np.isscalar(v) and np.isreal(v) and np.isfinite(v) and v > 0):
            raise ValueError(f"{name} must be positive and finite, not {v!r}")
    if not (np.isscalar(alpha) and np.isreal(alpha) and np.isfinite(alpha) and alpha >= 0):
        raise ValueError(f"alpha must be finite and not negative, not {alpha!r}")
    for name, v in (("beta_1", beta1), ("beta_2", beta2)):
        if not (np.isscalar(v) and np.isreal(v) and 0 <= v < 1):
            raise ValueError(f"{name} must lie in [0, 1), not {v!r}")
    if not (np.isscalar(tol) and np.isreal(tol) and np.isfinite(tol)):
        raise ValueError(f"tol must be finite, not {tol!r}")
    p = _lib.MlpFitParamsC()
    p.n_layers, p.hidden_activation, p.n_classes, p.batch_size = len(sizes) - 1, _lib.MLP_ACT[activation], int(n_classes), int(batch_size)
    p.max_epochs, p.n_iter_no_change = int(max_epochs), int(n_iter_no_change)
    for i, s in enumerate(sizes):
        p.sizes[i] = int(s)
    p.lr, p.alpha, p.beta1, p.beta2, p.epsilon, p.tol = float(lr), float(alpha), float(beta1), float(beta2), float(epsilon), float(tol)
    return p


def check_arrays(sizes, m, coefs, intercepts, mean, scale, order, max_epochs):
    """The host arrays of one fit as the library reads them: (coefs, intercepts, mean, scale, order), float32 copies of the weights
    (the call trains them in place)."""
    nl = len(sizes) - 1
    if len(coefs) != nl or len(intercepts) != nl:
        raise ValueError(f"{nl} layers need {nl} coefs and intercepts, not {len(coefs)} and {len(intercepts)}")
    W = [np.array(c, dtype=np.float32, order="C") for c in coefs]
    B = [np.array(b, dtype=np.float32, order="C") for b in intercepts]
    for l in range(nl):
        if W[l].shape != (sizes[l], sizes[l + 1]) or B[l].shape != (sizes[l + 1],):
            raise ValueError(f"layer {l}: coefs {W[l].shape} and intercepts {B[l].shape} do not fit the sizes {sizes[l]} -> {sizes[l + 1]}")
    out = []
    for name, v in (("mean", mean), ("scale", scale)):
        if v is not None:
            v = np.ascontiguousarray(v, dtype=np.float64)
            if v.shape != (sizes[0],):
                raise ValueError(f"{name} must hold one value per input column: shape ({sizes[0]},), not {v.shape}")
        out.append(v)
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int32)
        if order.shape != (max_epochs, m):
            raise ValueError(f"order must be the ({max_epochs}, {m}) table of the epochs' row orders, not {order.shape}")
        if order.size and (order.min() < 0 or order.max() >= m):
            raise ValueError(f"order names a row outside 0 .. {m - 1}")
    return W, B, out[0], out[1], order


def call(entry, handle, dist_ptr, m, ld, y_ptr, p, W, B, mean, scale, order, stream=None) -> FitResult:
    """One blocking call of wdx_mlp_fit_device (``stream`` given) or wdx_mlp_fit on checked arrays."""
    nl = p.n_layers
    cp = (C.c_void_p * nl)(*[w.ctypes.data for w in W])
    bp = (C.c_void_p * nl)(*[b.ctypes.data for b in B])
    curve = np.full(p.max_epochs, np.nan)
    n_epochs, state = C.c_int32(0), C.c_int32(0)
    args = [handle, dist_ptr, m, ld, y_ptr, C.byref(p), _lib.ptr(mean), _lib.ptr(scale), cp, bp, _lib.ptr(order), _lib.ptr(curve), C.byref(n_epochs),
            C.byref(state)]
    if stream is not None:
        args.append(stream)
    _lib.check(entry(*args))
    return FitResult(W, B, curve[:n_epochs.value].copy(), int(n_epochs.value), _lib.MLP_FIT_STATES[state.value])


def fit_host(dist, y_idx, p, W, B, mean, scale, order, device: Optional[int] = None) -> FitResult:
    """The fit on a float32 (m, F) HOST matrix through wdx_mlp_fit (the matrix is uploaded for the call)."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    y_idx = np.ascontiguousarray(y_idx, dtype=np.int32)
    ctx = _lib.default_context(device)
    return call(_lib.load().wdx_mlp_fit, ctx.handle, _lib.ptr(dist), dist.shape[0], dist.shape[1], _lib.ptr(y_idx), p, W, B, mean, scale, order)
