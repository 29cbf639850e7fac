"""The batched SMO solver on the device (include/wdx.h: wdx_svm_solve_device, wdx_svm_solve; DemuxEngine.svm_solve;
models.DTW_SVM.fit(solver="device")) against the rule restated in NumPy (tests/helpers/svm_fit_rule.py): alpha, rho, dec, n_iter
and state bit for bit.

The shapes are the smallest at which the kernel can go wrong: one row per side; 63 / 64 / 65 rows (a wave); one row more than an
instantiation's threads and than twice that, for each of the three instantiations (64, 256 and 1 024 threads -- 257 and 2 049 rows
are also the first sizes the next instantiation takes); 1 against 300; unequal bounds; C = 0.01 (no free row: rho's midpoint form);
duplicated rows (the 1e-12 branch); a kernel matrix that is not positive semi-definite (window-15 DTW from the device's own
self_distances); a scattered index list in a matrix with ld > m; 600 small problems in one launch; evaluation lists, empty and
not; an iteration cap of 10; one problem at the row cap.  The cap problem runs 150 iterations (state 1) and is compared bit for
bit like the others: the restatement is fast enough for that, so no weaker comparison is needed there."""
import ctypes as C
import functools
import json
import os
import sys
import time
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.abspath(__file__)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import kkt  # noqa: E402
from helpers import self_matrix_rule as sr  # noqa: E402
from helpers import stream_order as so  # noqa: E402
from helpers import svm_fit_rule as rule  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-3


def _imports():
    global torch, _lib, _svm_fit, DemuxEngine
    import torch
    from warpdemux_amd import _lib, _svm_fit
    from warpdemux_amd.engine import DemuxEngine


@pytest.fixture(scope="module")
def eng():
    _imports()
    e = DemuxEngine(np.random.default_rng(0).normal(size=(4, 25)), 15, 0.1)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _kernel(n, seed=0, noise=1.0, L=8, dup=0):
    """(K float32 (n, n) = exp(-Euclidean distance), y in {0, 1} sorted): two noisy classes; ``dup`` rows of each class are
    copies of the class's first row"""
    rng = np.random.default_rng(seed + 7 * n)
    y = (np.arange(n) >= n // 2).astype(int)
    X = rng.normal(size=(2, L))[y] + noise * rng.normal(size=(n, L))
    if dup:
        X[1:1 + dup] = X[0]
        X[n // 2 + 1:n // 2 + 1 + dup] = X[0]      # (copies of a row of the OTHER class too: K_ii + K_jj - 2 K_ij = 0 across the pair)
    D = np.sqrt(np.maximum(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1), 0.0)).astype(np.float32)
    K = np.exp(-D)
    K.setflags(write=False)
    return K, y


def _problems(specs):
    """specs: [(rows, n_pos, c_pos, c_neg, eval_rows)] -> (problem table, rows, eval_rows)"""
    tab, rows, evs, r0, e0 = [], [], [], 0, 0
    for r, n_pos, cp, cn, ev in specs:
        tab.append((r0, e0, n_pos, len(r) - n_pos, len(ev), 0, cp, cn))
        rows.append(np.asarray(r, np.int32)), evs.append(np.asarray(ev, np.int32))
        r0, e0 = r0 + len(r), e0 + len(ev)
    return np.array(tab, dtype=_svm_fit.PROBLEM_DTYPE), np.concatenate(rows), np.concatenate(evs)


def _check(eng, K, specs, eps=EPS, max_iter=10_000_000, Kd=None, stats=None, what=""):
    """the batch through DemuxEngine.svm_solve against the restatement, problem by problem -> the restatement's results"""
    tab, rows, evs = _problems(specs)
    if Kd is None:
        Kd = torch.tensor(K, device="cuda")
    res = eng.svm_solve(Kd, tab, rows, evs, eps=eps, max_iter=max_iter)
    alpha, rho, n_iter, state, dec = (t.cpu().numpy() for t in (res.alpha, res.rho, res.n_iter, res.state, res.dec))
    want = []
    for q, (r, n_pos, cp, cn, ev) in enumerate(specs):
        w = rule.solve(K, r, n_pos, cp, cn, eps, max_iter, ev, stats=stats)
        want.append(w)
        p = tab[q]
        tag = "%s problem %d (%d rows)" % (what, q, len(r))
        assert (int(state[q]), int(n_iter[q])) == (w.state, w.n_iter), (tag, int(state[q]), int(n_iter[q]), w.state, w.n_iter)
        got_a = alpha[p["row0"]:p["row0"] + len(r)]
        assert sr.same_bits(got_a, w.alpha), "%s: %d alpha differ, first at row %d" % (
            tag, int((sr.bits(got_a) != sr.bits(w.alpha)).sum()), int(np.argmax(sr.bits(got_a) != sr.bits(w.alpha))))
        assert sr.same_bits(rho[q:q + 1], np.array([w.rho])), (tag, "rho", rho[q], w.rho)
        assert sr.same_bits(dec[p["eval0"]:p["eval0"] + len(ev)], w.dec), (tag, "dec", dec[p["eval0"]:p["eval0"] + len(ev)][:4], w.dec[:4])
    return want


# ---- 1: sizes ---------------------------------------------------------------------------------------------------------------------------

SIZES = [2, 63, 64, 65, 129, 257, 513, 1025, 2049]


@pytest.mark.parametrize("n", SIZES)
def test_every_size_at_which_the_kernel_takes_another_path(eng, n):
    """n rows (n // 2 positive), and four evaluation rows from n = 63 on (rows of the same matrix behind the problem's)"""
    n_eval = 4 if n >= 63 else 0
    K, y = _kernel(n + n_eval, noise=0.7)
    spec = (np.r_[np.flatnonzero(y[:n] == 0), np.flatnonzero(y[:n] == 1)], int((y[:n] == 0).sum()), 1.0, 1.0, np.arange(n, n + n_eval))
    if n == 2:
        spec = (np.array([0, 1]), 1, 1.0, 1.0, np.zeros(0, int))
    t0 = time.time()
    w = _check(eng, K, [spec], what="n = %d" % n)[0]
    kern = next(k for k, (th, rpt) in enumerate(_lib.SVM_FIT_KERNELS) if th * rpt >= n)
    print("n", n, "instantiation", _lib.SVM_FIT_KERNELS[kern], "iterations", w.n_iter, "state", w.state, "support rows", int((w.alpha > 0).sum()),
          "seconds", round(time.time() - t0, 2))
    assert w.state == 0 and w.n_iter >= 1


def test_the_thresholds_between_the_instantiations_are_the_ones_tested():
    _imports()
    caps = [th * rpt for th, rpt in _lib.SVM_FIT_KERNELS]
    assert caps == [256, 2048, 16384] and caps[-1] == _lib.SVM_FIT_MAX_ROWS
    for th, _ in _lib.SVM_FIT_KERNELS:
        assert th + 1 in SIZES and 2 * th + 1 in SIZES
    assert caps[0] + 1 in SIZES and caps[1] + 1 in SIZES


# ---- 2: the rule's branches -------------------------------------------------------------------------------------------------------------

def test_one_against_three_hundred_and_unequal_bounds(eng):
    K, _ = _kernel(301, seed=1)
    specs = [(np.arange(301), 1, 1.0, 1.0, []), (np.arange(301), 1, 50.0, 0.25, [3]), (np.arange(301)[::-1].copy(), 300, 0.3, 2.0, []),
             (np.arange(300), 150, 2.0, 0.5, [300])]
    w = _check(eng, K, specs, what="1 vs 300")
    assert all(x.state == 0 for x in w)


def test_small_c_puts_every_row_at_its_bound_and_rho_is_the_midpoint(eng):
    K, _ = _kernel(200, seed=2, noise=1.0)
    stats = {}
    w = _check(eng, K, [(np.arange(200), 100, 0.01, 0.01, [0, 199])], stats=stats, what="C = 0.01")[0]
    assert stats["midpoint"] and (w.alpha == 0.01).all(), "built so that no row is free"


def test_duplicated_rows_take_the_tau_branch(eng):
    K, _ = _kernel(120, seed=3, noise=0.8, dup=6)
    stats = {}
    w = _check(eng, K, [(np.arange(120), 60, 1.0, 1.0, []), (np.arange(120), 60, 5.0, 5.0, [])], stats=stats, what="duplicates")
    print("pairs on the 1e-12 branch", stats.get("tau", 0), "iterations", [x.n_iter for x in w])
    assert stats.get("tau", 0) >= 1, "built so that a pair of identical rows of opposite classes is selected"


def test_a_kernel_matrix_that_is_not_positive_semidefinite(eng):
    """K = exp(-0.1 D) of window-15, penalty-0.1 DTW distances from the device's own self_distances (gamma = 0.1: at gamma = 1
    these rows' matrix is diagonally dominant, smallest eigenvalue 0.79; at 0.1 it is -0.04): it stays on the device for the solve;
    the restatement reads a host copy"""
    Xtr, y, _, _ = sr.training_rows(2, 220, 25, 9)
    Kd = torch.exp(-0.1 * eng.self_distances(torch.from_numpy(Xtr).cuda(), 15, 0.1)).contiguous()
    K = Kd.cpu().numpy()
    lam = float(np.linalg.eigvalsh(K.astype(np.float64)).min())
    print("smallest eigenvalue", lam)
    assert lam < -1e-6, "the input was built not to be positive semi-definite"
    rows = np.r_[np.flatnonzero(y == 0), np.flatnonzero(y == 1)]
    w = _check(eng, K, [(rows, int((y == 0).sum()), 1.0, 1.0, []), (rows, int((y == 0).sum()), 100.0, 100.0, [])], Kd=Kd, what="DTW kernel")
    print("iterations", [x.n_iter for x in w], "states", [x.state for x in w])


def test_scattered_index_list_and_a_leading_dimension_beyond_m(eng):
    K, y = _kernel(400, seed=4)
    wide = torch.full((400, 437), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :400] = torch.tensor(K, device="cuda")
    rng = np.random.default_rng(1)
    pos, neg = rng.permutation(np.flatnonzero(y == 0))[:70], rng.permutation(np.flatnonzero(y == 1))[:55]
    rest = np.setdiff1d(np.arange(400), np.r_[pos, neg])[:9]
    w = _check(eng, K, [(np.r_[pos, neg], 70, 1.0, 1.5, rest)], Kd=wide[:, :400], what="scattered rows, ld 437")[0]
    assert w.state == 0 and not np.isnan(w.dec).any(), "a NaN of the gap columns reached a result"


def test_six_hundred_small_problems_in_one_launch(eng):
    K, y = _kernel(64, seed=5)
    rng = np.random.default_rng(2)
    specs = []
    for q in range(600):
        npos, nneg = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        pos, neg = rng.choice(np.flatnonzero(y == 0), npos, replace=False), rng.choice(np.flatnonzero(y == 1), nneg, replace=False)
        ev = rng.choice(64, int(rng.integers(0, 4)), replace=False) if q % 3 else []
        specs.append((np.r_[pos, neg], npos, float(rng.choice([0.1, 1.0, 10.0])), float(rng.choice([0.1, 1.0, 10.0])), ev))
    w = _check(eng, K, specs, what="600 problems")
    assert sum(len(s[4]) == 0 for s in specs) >= 200 and sum(len(s[4]) > 0 for s in specs) >= 200, "empty and non-empty evaluation lists"
    assert all(x.state == 0 for x in w)


def test_iteration_cap_of_ten_gives_state_one_and_the_alpha_reached(eng):
    K, _ = _kernel(300, seed=6)
    w = _check(eng, K, [(np.arange(300), 150, 1.0, 1.0, [0, 7]), (np.arange(40), 20, 1.0, 1.0, [])], max_iter=10, what="max_iter 10")
    assert (w[0].state, w[0].n_iter) == (1, 10) and int((w[0].alpha > 0).sum()) <= 20
    zero = _check(eng, K, [(np.arange(300), 150, 1.0, 1.0, [])], max_iter=0, what="max_iter 0")[0]
    assert (zero.state, zero.n_iter) == (1, 0) and (zero.alpha == 0).all()


def test_one_problem_at_the_row_cap_and_one_row_beyond_is_refused(eng):
    """16 384 rows: every slot of every thread of the largest instantiation and all of its LDS.  The matrix is built on the device;
    150 iterations (state 1), bit for bit against the restatement on a host copy."""
    n = _lib.SVM_FIT_MAX_ROWS
    g = torch.Generator(device="cuda").manual_seed(5)
    y = (torch.arange(n + 3, device="cuda") >= n // 2).double()
    X = 0.8 * y[:, None] + torch.randn((n + 3, 6), generator=g, device="cuda", dtype=torch.float64)
    Kd = torch.exp(-torch.cdist(X, X)).float().contiguous()
    del X
    K = Kd.cpu().numpy()
    t0 = time.time()
    w = _check(eng, K, [(np.arange(n), n // 2, 1.0, 2.0, [n, n + 1, n + 2])], max_iter=150, Kd=Kd, what="the cap")[0]
    print("cap: state", w.state, "iterations", w.n_iter, "support rows", int((w.alpha > 0).sum()), "seconds", round(time.time() - t0, 2))
    assert (w.state, w.n_iter) == (1, 150) and int((w.alpha > 0).sum()) >= 2
    tab, rows, evs = _problems([(np.zeros(n + 1, int), 5, 1.0, 1.0, [])])
    with pytest.raises(NotImplementedError, match="16385 rows, more than WDX_SVM_FIT_MAX_ROWS = 16384"):
        eng.svm_solve(Kd, tab, rows, evs)
    out = [torch.full((n + 1,), 7.0, dtype=torch.float64, device="cuda"), torch.full((1,), 7.0, dtype=torch.float64, device="cuda"),
           torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), 9, dtype=torch.int32, device="cuda")]
    rc = eng.L.wdx_svm_solve_device(eng.ctx.handle, C.c_void_p(Kd.data_ptr()), n + 3, n + 3, _lib.ptr(tab), 1, _lib.ptr(rows), len(rows), None, 0, EPS,
                                    100, *[C.c_void_p(t.data_ptr()) for t in out], None, None)
    assert rc == _lib.WDX_ERR_INVALID and "has 16385 rows, more than WDX_SVM_FIT_MAX_ROWS = 16384" in eng.L.wdx_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out[0] == 7.0).all()) and int(out[3][0]) == 9, "a refused call wrote an output"


# ---- 3: a NaN ends the solve; refusals --------------------------------------------------------------------------------------------------

def test_a_nan_in_k_ends_the_solve_with_state_two(eng):
    """through the device entry (the host form refuses such a K): the NaN sits in the row the first iteration reads, so the
    gradient of one row stops being finite and the second iteration's check ends the solve"""
    K0, _ = _kernel(150, seed=8)
    K = K0.copy()
    K[0, 5] = np.nan
    w = _check(eng, K, [(np.arange(150), 75, 1.0, 1.0, [1, 2]), (np.arange(10, 150), 65, 1.0, 1.0, [3])], what="NaN in K")
    assert (w[0].state, w[0].n_iter) == (2, 1) and np.isnan(w[0].rho) and np.isnan(w[0].dec).all()
    assert w[1].state == 0, "the problem that never reads the entry converges"
    tab, rows, evs = _problems([(np.arange(150), 75, 1.0, 1.0, [1])])
    out = _svm_fit.Solution(np.zeros(150), np.empty(1), np.empty(1, np.int64), np.empty(1, np.int32), np.zeros(1))
    with pytest.raises(ValueError, match=r"K\[0, 5\] is not finite"):
        _lib.check(eng.L.wdx_svm_solve(eng.ctx.handle, _lib.ptr(K), 150, 150, _lib.ptr(tab), 1, _lib.ptr(rows), 150, _lib.ptr(evs), 1, EPS, 100,
                                       *[_lib.ptr(a) for a in out]))


def test_bad_problems_are_refused_before_a_launch_and_the_context_stays_usable(eng):
    K, _ = _kernel(40, seed=9)
    Kd = torch.tensor(K, device="cuda")
    out = [torch.full((40,), 7.0, dtype=torch.float64, device="cuda"), torch.full((1,), 7.0, dtype=torch.float64, device="cuda"),
           torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), 9, dtype=torch.int32, device="cuda"),
           torch.full((2,), 7.0, dtype=torch.float64, device="cuda")]

    def call(spec, m=40, ld=40, eps=EPS, max_iter=100, K_=Kd, outs=out):
        tab, rows, evs = _problems([spec])
        rc = eng.L.wdx_svm_solve_device(eng.ctx.handle, None if K_ is None else C.c_void_p(K_.data_ptr()), m, ld, _lib.ptr(tab), 1, _lib.ptr(rows),
                                        len(rows), _lib.ptr(evs), len(evs), eps, max_iter, *[None if t is None else C.c_void_p(t.data_ptr()) for t in outs], None)
        return rc, eng.L.wdx_last_error().decode()

    good = (np.arange(40), 20, 1.0, 1.0, [0, 1])
    for spec, kw, needle in (
            ((np.r_[np.arange(39), 40], 20, 1.0, 1.0, []), {}, "row 39 is K row 40, outside 0 .. 39"),
            ((np.r_[-1, np.arange(39)], 20, 1.0, 1.0, []), {}, "row 0 is K row -1"),
            ((np.arange(40), 20, 1.0, 1.0, [40]), {}, "evaluation row 0 is K row 40"),
            ((np.arange(40), 40, 1.0, 1.0, []), {}, "has an empty side (n_pos = 40, n_neg = 0)"),
            ((np.arange(40), 0, 1.0, 1.0, []), {}, "has an empty side"),
            ((np.arange(40), 20, 0.0, 1.0, []), {}, "must be positive and finite"),
            ((np.arange(40), 20, 1.0, float("inf"), []), {}, "must be positive and finite"),
            ((np.arange(40), 20, 1.0, float("nan"), []), {}, "must be positive and finite"),
            (good, dict(ld=39), "ld = 39 is less than m = 40"),
            (good, dict(eps=0.0), "eps must be positive and finite"),
            (good, dict(max_iter=-1), "max_iter must not be negative"),
            (good, dict(K_=None), "the kernel matrix is required"),
            (good, dict(outs=out[:4] + [None]), "has evaluation rows and dec is NULL"),
            (good, dict(outs=[None] + out[1:]), "alpha, rho, n_iter and state are required")):
        rc, msg = call(spec, **kw)
        assert rc == _lib.WDX_ERR_INVALID and needle in msg, (needle, rc, msg)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (out[0], out[1], out[4])) and int(out[3][0]) == 9, "a refused call wrote an output"
    with pytest.raises(ValueError, match="K must be a float32 device tensor"):
        eng.svm_solve(Kd.double(), *_problems([good]))
    empty = eng.svm_solve(Kd, np.zeros(0, _svm_fit.PROBLEM_DTYPE), np.zeros(0, np.int32))
    assert tuple(empty.rho.shape) == (0,)
    _check(eng, K, [good], what="after the refusals")


# ---- 4: DTW_SVM.fit(solver="device") ------------------------------------------------------------------------------------------------------

def test_fit_on_the_device_against_the_libsvm_fit():
    """600 rows, 4 classes, L 25, window 15, C = 1, class_weight="balanced" (the recipe of the shipped models), one row dropped.
    Asserted: the KKT bound on the device model (the project's helper on the support rows, the all-rows helper per pair), the same
    label_mapper and n_dropped_, and that predict runs on the resident tail.  Printed, not asserted: the differences to the libsvm
    fit's decision values and probA / probB (the folds are this engine's own)."""
    _imports()
    from warpdemux_amd import parallel_distances as pdist
    from warpdemux_amd.models import DTW_SVM

    Xtr, y, Xte, yte = sr.training_rows(4, 601, 25, 21)
    Xtr = Xtr.copy()
    Xtr[17, 3] = np.nan
    labels = np.arange(4) * 3 + 2
    keep = np.isfinite(Xtr).all(axis=1)
    D = pdist.self_distance_matrix(np.ascontiguousarray(Xtr[keep]), 15, 0.1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # (a problem that did not converge would warn)
        t0 = time.time()
        dev = DTW_SVM.fit(Xtr, labels[y], 15, 0.1, class_weight="balanced", solver="device")
        t1 = time.time()
        ref = DTW_SVM.fit(Xtr, labels[y], 15, 0.1, class_weight="balanced", solver="libsvm")
        t2 = time.time()
    assert dev.label_mapper == ref.label_mapper == {i: int(c) for i, c in enumerate(labels)} and dev.n_dropped_ == ref.n_dropped_ == 1
    assert np.array_equal(dev._X, ref._X) and (dev.fit_info_["state"] == 0).all() and len(dev.fit_info_["state"]) == 36
    ym = y[keep]
    w = len(ym) / (4 * np.bincount(ym).astype(np.float64))
    sup = dev._support
    res = kkt.kkt_residuals(D[np.ix_(sup, sup)], dev._n_support, dev._dual_coef, -dev._rho, w)
    K = np.exp(-D)
    where = np.full(len(ym), -1)
    where[sup] = np.arange(len(sup))
    worst_all = 0.0
    for p, (i, j) in enumerate(dev.fit_info_["pairs"]):
        rows = np.r_[np.flatnonzero(ym == i), np.flatnonzero(ym == j)]
        n_pos = int((ym == i).sum())
        coef = np.where(where[rows] >= 0, np.where(np.arange(len(rows)) < n_pos, dev._dual_coef[j - 1, where[rows]], dev._dual_coef[i, where[rows]]), 0.0)
        worst_all = max(worst_all, rule.kkt_worst(K, rows, n_pos, w[i], w[j], np.abs(coef), dev._rho[p]))
    print("device fit", round(t1 - t0, 3), "s, libsvm fit", round(t2 - t1, 3), "s; support rows", len(sup), "of", len(ym), "(libsvm:", len(ref._support), ")")
    print("worst KKT residual: support rows", kkt.worst(res), "all rows", worst_all, "iterations", dev.fit_info_["n_iter"].tolist())
    assert kkt.worst(res) <= kkt.EPS_LIBSVM and worst_all <= kkt.EPS_LIBSVM
    # the differences to the libsvm fit, printed: pairwise decision values of the held-out rows, probA / probB
    Kq = np.exp(-pdist.distance_matrix_to(Xte, dev._X, window=15, penalty=0.1, n_jobs=1)).astype(np.float64)
    dec = lambda m: np.stack([Kq[:, m._support] @ c for c in m._dual_coef])   # noqa: E731  (per coefficient row; the pairs mix two rows)
    print("max |coefficient-row sums - libsvm's|", float(np.abs(dec(dev) - dec(ref)).max()) if np.array_equal(dev._support, ref._support) else "support rows differ",
          "max |rho - libsvm's|", float(np.abs(dev._rho - ref._rho).max()))
    print("max |probA - libsvm's|", float(np.abs(dev._probA - ref._probA).max()), "max |probB - libsvm's|", float(np.abs(dev._probB - ref._probB).max()))
    y_pred, y_prob = dev.predict(Xte, nproc=1)
    y_ref, p_ref = ref.predict(Xte, nproc=1)
    print("accuracy device", float((y_pred == labels[yte]).mean()), "libsvm", float((y_ref == labels[yte]).mean()), "max |prob - libsvm's|", float(np.abs(y_prob - p_ref).max()))
    assert y_prob.shape == (256, 4) and np.isfinite(y_prob).all() and np.allclose(y_prob.sum(axis=1), 1.0) and np.isin(y_pred, labels).all()


# ---- 5: the stream contract ---------------------------------------------------------------------------------------------------------------

def test_device_entry_enqueues_on_the_callers_stream_without_waiting():
    """the pattern of tests/test_gpu_streams.py: on a side stream whose kernel matrix arrives LATE (the tensor holds a decoy until,
    behind a device-side delay, the real matrix is copied in) the call returns while the delay is still running and gives the
    serial call's results bit for bit; a fresh child process, which first proves that its side streams overtake"""
    res, _ = so.run_child(HERE, ["stream"], timeout=150.0)
    assert res.get("ok") is True and res["same"] and res["pending"] and res["decoy_differs"], res


def _child_stream():
    _imports()
    A, B, log = so.side_streams()
    print("\n".join(log))
    K, _ = _kernel(300, seed=6)
    Kw, _ = _kernel(300, seed=16, noise=0.5)
    e, ref = (DemuxEngine(np.zeros((4, 25)), 15, 0.1) for _ in range(2))
    tab, rows, evs = _problems([(np.arange(300), 150, 1.0, 1.0, [0, 7]), (np.arange(100, 300), 50, 2.0, 1.0, [5])])
    real, decoy = torch.tensor(K, device="cuda"), torch.tensor(Kw, device="cuda")
    flat = lambda r: np.concatenate([t.cpu().numpy().view(np.uint8).ravel() for t in (r.alpha, r.rho, r.n_iter, r.state, r.dec)])   # noqa: E731
    serial, wrong = flat(ref.svm_solve(real, tab, rows, evs)), flat(ref.svm_solve(decoy, tab, rows, evs))
    e.svm_solve(real, tab, rows, evs)                      # warm: tables sized, kernel loaded
    torch.cuda.synchronize()
    t0 = time.time()
    e.svm_solve(real, tab, rows, evs)
    torch.cuda.synchronize()
    ms = so.delay_ms_for(time.time() - t0)
    Kt = torch.empty_like(real)
    ev = so.late(A, [Kt], [real], [decoy], ms)
    with torch.cuda.stream(A):
        res = e.svm_solve(Kt, tab, rows, evs)
        pending = not ev.query()                           # the call came back with the delay still running
        got = flat(res)                                    # (copies on A: they wait for A alone)
    e.close(), ref.close()
    print(json.dumps(dict(ok=True, same=bool(np.array_equal(got, serial)), pending=pending, decoy_differs=not np.array_equal(wrong, serial), delay_ms=ms)))


if __name__ == "__main__":
    if sys.argv[1:] == ["stream"]:
        _child_stream()
