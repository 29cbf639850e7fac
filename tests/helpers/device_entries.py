"""The table of the `wdx_*_device` entries (include/wdx.h): the training entries whose arrays live on the device.  One row per
export; tests/test_device_entry_table_host.py closes the table in both directions (every `_device` name of `_lib.EXPORTS`, every
`wdx_\\w+_device(` prototype of the header), tests/test_gpu_device_entries.py runs every case of every row in exact frames
(tests/helpers/framed.py).  The sibling table of the `_dev` entries is in tests/test_gpu_buffer_bounds.py.

A row (`Entry`) names its arguments by role, the `DemuxEngine` method that answers the same call, the NumPy rule that restates it,
and builds its cases.  A `Case` holds, for one call:

    inputs    name -> the exact documented elements (a flat array for a matrix with a leading dimension: it ends on element
              (m-1) * ld + cols - 1, and its pad columns hold NaN)
    inouts    name -> the same for an array the call reads and writes (d_scores; d_D of an in-place kernel matrix)
    outputs   name -> (elements, dtype): the exact documented size
    written   name -> a bool mask over the flat elements: False where the header says "not written" (default: all written)
    nullable  the outputs that may be NULL (all given, then all NULL: the outputs that remain keep their bits)
    null_in   the inputs handed over as NULL in this case
    call      (L, handle, p, stream) -> dict of HOST outputs; p maps every device argument to its pointer (None: NULL)
    engine    (eng, t) -> dict name -> device tensor (a matrix with a leading dimension as its whole (rows, ld) tensor) or host array,
              through the DemuxEngine method on roomy tensors (a row with second = "ctypes": through the same entry, as
              wdx_svm_cv_couple_device, whose method svm_cross_val does far more than this call), without a synchronisation of its own; t = `tensors(torch, case)`;
              `finish(case, d)` brings the dict into the payload's layout on the host
    rule      () -> the same dict from the NumPy rule, or None where the row says why there is none
    check     (got) -> None: further assertions of the case on the outputs (flat arrays by name)
    options   ((option, value), ...) set on both contexts for the case
    big       a Case of the same entry at a larger, different shape: what a "leftover" context has just run

Shapes are the smallest at which each kernel can still go wrong; the constants they come from are restated below and pinned to the
sources by the host test.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Callable, NamedTuple

import numpy as np

from . import boost_fit_rule, dba_rule, loo_rule, medoid_rule, self_matrix_rule, svm_cv_rule, svm_fit_rule, svm_ref

IN, IN_NULLABLE, OUT, OUT_NULLABLE, INOUT, HOST, HOST_OUT = "in", "in?", "out", "out?", "inout", "host", "host out"

L_DTW, WINDOW, PENALTY = 25, 15, 0.1

# kernel constants the shapes below stand on, restated (tests/test_device_entry_table_host.py pins each to its source)
CHUNK_ROWS = 64                # wdx_medoid_plan.h: kMedoidChunk, rows of one tile chunk
SVM_KERNEL_COLS = 1024         # wdx_svm_kernel.hip: kSvmKernelThreads * kSvmKernelPerThread columns per workgroup
SVM_KERNEL_VEC = 4             # ... kSvmKernelPerThread: entries of one 16-byte access
CV_ROWS_PER_WAVE = 4           # wdx_svm_cv.hip: 16-lane groups of a one-wave workgroup
CV_GROUP_LANES = 16            # ... lanes that gather a row's pairs: more than one trip from k = 7 on (21 pairs)
CV_CLASSES = (2, 7, 16)
THR_ROWS = 4096                # wdx_thresholds_plan.h: kThrRows
THR_LDS_ENTRIES = 12288        # ... kThrLdsEntries: 2 (R + 1) counters a class; k = 16 needs a second class group from R = 384 on
THR_SELECT_BINS = 64           # wdx_thresholds.hip: bins per step of the select kernel
MLP_FIT_ROWS = 16              # wdx_mlp_fit_plan.h: kMlpFitRows, rows of one workgroup
BOOST_FIT_ROWS = 2047          # include/wdx.h: WDX_BOOST_FIT_ROWS

DTW_MAX_REG_WINDOW = 32        # wdx_dtw_plan.h: kMaxRegWindow, the widest band the register kernels serve

OPT_DBA_GENERAL, OPT_SELF_NEAREST_GENERAL = 27, 28   # (_lib names them; restated so that this module imports without the library)


class Arg(NamedTuple):
    name: str
    role: str
    what: str     # the documented size


class Case:
    def __init__(self, id, call, engine, rule=None, inputs=None, inouts=None, outputs=None, written=None, nullable=(), null_in=(),
                 check=None, options=(), big=None, offsets=None, null_big=False):
        self.id, self.call, self.engine, self.rule, self.check = id, call, engine, rule, check
        self.inputs, self.inouts, self.outputs = dict(inputs or {}), dict(inouts or {}), dict(outputs or {})
        self.written, self.nullable, self.null_in, self.options = dict(written or {}), tuple(nullable), tuple(null_in), tuple(options)
        self.big = big                    # a callable: built only when a leftover context is wanted
        self.offsets = dict(offsets or {})   # name -> bytes added to the frame's offset (wdx_svm_kernel_device's base pointers)
        self.null_big = null_big          # the leftover call runs with its nullable outputs NULL (the context's own histograms)
        self.matrix = {}                  # name -> (rows, ld, cols) of an input or in/out matrix with a leading dimension

    def __repr__(self):
        return self.id


class Entry(NamedTuple):
    name: str
    args: tuple            # of Arg
    engine: str            # the DemuxEngine method that makes this call
    rule: str              # the NumPy rule, or why there is none
    cases: Callable        # () -> [Case]
    second: str = "method"  # how the second context answers: through `engine` ("method"), or through the same ctypes entry on roomy
                            # tensors ("ctypes": the method does more than the bare call)


def vp(v):
    return None if v is None else C.c_void_p(int(v))


def pack(M, ld, cols=None, pad=np.nan):
    """the flat documented elements of a (rows, cols) matrix with leading dimension ld: (rows-1) * ld + cols of them, `pad` between
    the rows"""
    M = np.asarray(M)
    rows, cols = M.shape[0], (M.shape[1] if cols is None else cols)
    out = np.full((rows - 1) * ld + cols if rows else 0, pad, dtype=M.dtype)
    for r in range(rows):
        out[r * ld:r * ld + cols] = M[r, :cols]
    return out


def pack_mask(rows, ld, cols):
    return pack(np.ones((rows, cols), dtype=bool), ld, cols, pad=False)


def roomy(torch, flat, rows, ld, cols):
    """the (rows, cols) view of a (rows, ld) device tensor that holds a packed matrix (NaN in every pad, the last row's included)"""
    flat = np.asarray(flat)
    full = np.full(rows * ld, np.nan, dtype=flat.dtype)
    full[:flat.size] = flat
    return torch.from_numpy(full).cuda().view(rows, ld)[:, :cols]


def _flat(a):
    return None if a is None else np.ascontiguousarray(a).reshape(-1)


def tensors(torch, case, values=None):
    """name -> the device tensor DemuxEngine takes for every input and in/out array of the case (a matrix with a leading dimension as
    the (rows, cols) view of its (rows, ld) tensor, the whole tensor under name + ":full"); ``values``: other flat arrays of the same
    sizes (a decoy)"""
    t = {}
    for name, a in {**case.inputs, **case.inouts}.items():
        a = a if values is None else values[name]
        if name in case.matrix:
            t[name] = roomy(torch, a, *case.matrix[name])
            t[name + ":full"] = t[name]._base
        else:
            t[name] = torch.from_numpy(np.array(a)).cuda()
    return t


def finish(case, d):
    """what `case.engine` returned, on the host: every array flat and cut to the documented elements (a (rows, ld) tensor loses the pad
    behind its last row)"""
    out = {}
    for name, v in d.items():
        a = _flat(v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v))
        size = case.outputs[name][0] if name in case.outputs else (case.inouts[name].size if name in case.inouts else a.size)
        out[name] = a[:size]
    return out


# ---- the DTW entries -------------------------------------------------------------------------------------------------------------

def _labelled(sizes, L, seed, minus=8):
    """(X (n, L), labels int32 (n,)): rows around one random-walk centre per label, `minus` rows labelled -1, in shuffled row order"""
    rng = np.random.default_rng(seed)
    lab = np.concatenate([np.full(m, g) for g, m in enumerate(sizes)] + [np.full(minus, -1)]).astype(np.int32)
    rng.shuffle(lab)
    X = np.empty((lab.size, L))
    for g in list(range(len(sizes))) + [-1]:
        q = np.flatnonzero(lab == g)
        c = np.cumsum(rng.normal(0, 0.6, L))
        X[q] = (c - c.mean()) / (c.std() + 1e-9) + rng.normal(0, 0.35, (len(q), L))
    return X, lab


def _medoid_case(id, sizes, L, window, with_status, seed, big=None):
    X, lab = _labelled(sizes, L, seed)
    n, G = len(lab), len(sizes)
    status = np.zeros(n, np.int32)
    X[np.flatnonzero(lab == 3)[4], L // 3] = np.nan                 # a NaN row: no member
    status[np.flatnonzero(lab == 4)[0]] = 1                          # a member only when d_status is NULL
    st = status if with_status else None

    def call(Lb, h, p, stream):
        from warpdemux_amd import _lib
        _lib.check(Lb.wdx_medoids_device(h, vp(p["dX"]), n, L, _lib.ptr(lab), G, vp(p["d_status"]), window, PENALTY, vp(p["d_medoid"]),
                                         vp(p["d_medoid_cost"]), vp(p["d_count"]), vp(p["d_cost"]), vp(p["d_refs"]), stream))
        return {}

    def engine(eng, t):
        r = eng.medoids(t["dX"].view(n, L), lab, G, window=window, penalty=PENALTY, status=t.get("d_status"), want_cost=True)
        return dict(d_medoid=r.index, d_medoid_cost=r.medoid_cost, d_count=r.count, d_cost=r.cost, d_refs=r.refs)

    def rule():
        r = medoid_rule.medoid_rule(X, lab, G, window, PENALTY, st)
        return dict(d_medoid=r["index"], d_medoid_cost=r["medoid_cost"], d_count=r["count"], d_cost=r["cost"], d_refs=_flat(r["refs"]))

    inputs = dict(dX=_flat(X))
    if with_status:
        inputs["d_status"] = status
    return Case(id, call, engine, rule, inputs=inputs, null_in=() if with_status else ("d_status",),
                outputs=dict(d_medoid=(G, "int64"), d_medoid_cost=(G, "float64"), d_count=(G, "int64"), d_cost=(n, "float64"),
                             d_refs=(G * L, "float64")),
                nullable=("d_medoid_cost", "d_count", "d_cost", "d_refs"), big=big)


def medoid_cases():
    """L = 25, window 15, 135 rows: label 0 of 65 rows (two chunks of 64), label 1 of one row, label 2 without a row, label 3 with a NaN
    row, label 4's only row with status 1 (no member: a label without one, unless d_status is NULL), 8 rows labelled -1"""
    big = lambda: _medoid_case("big", (150, 130, 0, 100, 3), 31, 9, True, 5)   # noqa: E731
    return [_medoid_case("status" if s else "no-status", (CHUNK_ROWS + 1, 1, 0, 60, 1), L_DTW, WINDOW, s, 3, big) for s in (True, False)]


def _self_matrix_case(id, n, ld, L, seed, big=None):
    X, status = self_matrix_rule.rows(L, n, seed)
    cells = (n - 1) * ld + n

    def call(Lb, h, p, stream):
        from warpdemux_amd import _lib
        _lib.check(Lb.wdx_self_matrix_device(h, vp(p["dX"]), n, L, vp(p["d_status"]), WINDOW, PENALTY, vp(p["d_out"]), ld, stream))
        return {}

    def engine(eng, t):
        import torch
        out = torch.zeros((n, ld), dtype=torch.float32, device="cuda")
        eng.self_distances(t["dX"].view(n, L), WINDOW, PENALTY, status=t["d_status"], out=out[:, :n])
        return dict(d_out=out)

    return Case(id, call, engine, lambda: dict(d_out=pack(self_matrix_rule.self_matrix_rule(X, WINDOW, PENALTY, status), ld, n, pad=0)),
                inputs=dict(dX=_flat(X), d_status=status), outputs=dict(d_out=(cells, "float32")), written=dict(d_out=pack_mask(n, ld, n)), big=big)


def self_matrix_cases():
    """n = 1 and n = 65 (a second chunk of one row), ld = n and n + 3: columns n .. ld-1 keep what they held"""
    big = lambda: _self_matrix_case("big", 200, 203, 31, 4)   # noqa: E731
    return [_self_matrix_case("n%d-ld%d" % (n, n + e), n, n + e, L_DTW, 11, big) for n in (1, CHUNK_ROWS + 1) for e in (0, 3)]


def _self_nearest_case(id, n, L, with_labels, general, seed, big=None):
    X, labels, status = loo_rule.rows(L, n, seed)
    if n < 130:
        labels[7] = 5            # the only row of its label: own side -1 / +inf
        X[11, 2] = np.nan
        labels[20] = -1
    status[3] = 1
    lab = labels if with_labels else None

    def call(Lb, h, p, stream):
        from warpdemux_amd import _lib
        _lib.check(Lb.wdx_self_nearest_device(h, vp(p["dX"]), n, L, vp(p["d_label"]), vp(p["d_status"]), WINDOW, PENALTY, vp(p["d_nn"]),
                                              vp(p["d_best"]), stream))
        return {}

    def engine(eng, t):
        r = eng.loo_nearest(t["dX"].view(n, L), t.get("d_label"), window=WINDOW, penalty=PENALTY, status=t["d_status"])
        return dict(d_nn=r.nn, d_best=r.best)

    def rule():
        nn, best = loo_rule.loo_rule(X, lab, WINDOW, PENALTY, status)
        return dict(d_nn=_flat(nn), d_best=_flat(best))

    inputs = dict(dX=_flat(X), d_status=status)
    if with_labels:
        inputs["d_label"] = labels
    return Case(id, call, engine, rule, inputs=inputs, null_in=() if with_labels else ("d_label",),
                outputs=dict(d_nn=(2 * n, "int32"), d_best=(2 * n, "float32")), options=((OPT_SELF_NEAREST_GENERAL, int(general)),), big=big)


def self_nearest_cases():
    """n = 65 and 130 (a second and a third chunk), labels given and NULL, a label with a single member, the tile route and the
    general one"""
    big = lambda g: (lambda: _self_nearest_case("big", 200, 31, True, g, 2))   # noqa: E731
    return [_self_nearest_case("n%d-%s-%s" % (n, "labels" if wl else "no-labels", "general" if g else "tiles"), n, L_DTW, wl, g, 29, big(g))
            for n in (CHUNK_ROWS + 1, 2 * CHUNK_ROWS + 2) for wl in (True, False) for g in (0, 1)]


def _dba_case(id, sizes, L, window, general, seed, big=None):
    X, lab = _labelled(sizes, L, seed, minus=4)
    n, G = len(lab), len(sizes)
    rng = np.random.default_rng(seed + 1)
    status = np.zeros(n, np.int32)
    status[np.flatnonzero(lab == 0)[3]] = 1
    X[np.flatnonzero(lab == 1)[2], L - 1] = np.inf
    centres = np.stack([X[np.flatnonzero(lab == g)[-1]] if (lab == g).any() else rng.normal(size=L) for g in range(G)]) + rng.normal(0, 0.1, (G, L))
    win = window or 0

    def call(Lb, h, p, stream):
        from warpdemux_amd import _lib
        _lib.check(Lb.wdx_dba_step_device(h, vp(p["dX"]), n, L, _lib.ptr(lab), G, vp(p["d_status"]), vp(p["d_centres"]), win, PENALTY,
                                          vp(p["d_new"]), vp(p["d_count"]), vp(p["d_inertia"]), vp(p["d_cost"]), vp(p["d_runs"]), stream))
        return {}

    def engine(eng, t):
        r = eng.dba_step(t["dX"].view(n, L), lab, t["d_centres"].view(G, L), G, window=window, penalty=PENALTY, status=t["d_status"],
                         want_cost=True, want_runs=True)
        return dict(d_new=r.centres, d_count=r.count, d_inertia=r.inertia, d_cost=r.cost, d_runs=r.runs)

    def rule():
        r = dba_rule.dba_step(X, lab, centres, G, window, PENALTY, status)
        return dict(d_new=_flat(r["new_centres"]), d_count=r["count"], d_inertia=r["inertia"], d_cost=r["cost"], d_runs=_flat(r["runs"]))

    return Case(id, call, engine, rule, inputs=dict(dX=_flat(X), d_status=status, d_centres=_flat(centres)),
                outputs=dict(d_new=(G * L, "float64"), d_count=(G, "int64"), d_inertia=(G, "float64"), d_cost=(n, "float64"),
                             d_runs=(2 * n * L, "int32")),
                nullable=("d_count", "d_inertia", "d_cost", "d_runs"), options=((OPT_DBA_GENERAL, int(general)),), big=big)


def dba_cases():
    """131 rows, L = 25: a label of 65 rows (two chunks), one idle label (no row); window 15 on the register band, and window 0 on
    the general route (dba_align_general_kernel and the `rolling` piece of the workspace).  Unbanded L = 25 is an effective window of
    25, which the band ladder still serves (wdx_dba_plan.h: dba_kernel), so that case and its leftover call run with
    WDX_OPT_DBA_GENERAL = 1; tests/test_device_entry_table_host.py pins both routes.  d_count, d_inertia, d_cost and d_runs given and
    NULL"""
    big = lambda w, g: (lambda: _dba_case("big", (200, 186, 0), 31, w and 9, g, 8))   # noqa: E731
    return [_dba_case("window%d-%s" % (w, "general" if g else "band"), (CHUNK_ROWS + 1, 40, 0, 22), L_DTW, w, g, 6, big(w, g))
            for w, g in ((WINDOW, 0), (0, 1))]


# ---- the kernel machine ----------------------------------------------------------------------------------------------------------------

def _kernel_of(m, k, seed, L=6):
    rng = np.random.default_rng(seed)
    y = np.sort(rng.integers(0, k, m))
    y[:k] = np.arange(k)
    y = rng.permutation(y)
    X = rng.normal(size=(k, L))[y] + 0.9 * rng.normal(size=(m, L))
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    return np.exp(-0.5 * D), y


SVM_SOLVE_M, SVM_SOLVE_LD, SVM_SOLVE_EPS = 40, 41, 1e-3


@functools.lru_cache(maxsize=None)
def svm_solve_batch(m=SVM_SOLVE_M, k=3, seed=12, nan=True):
    """(K (m, m) float32, Batch, max_iter): the k (k - 1) / 2 full problems and their Platt folds with evaluation rows; max_iter is the
    median of the problems' iteration counts (the longer ones end in state 1), and a NaN sits in K where the LAST pair's first
    iteration reads it (its problems end in state 2, the other pairs never name both rows)"""
    from warpdemux_amd import _svm_fit
    K, y = _kernel_of(m, k, seed)
    batch = _svm_fit.build_batch(y, k, np.ones(k), random_state=1, folds=True)
    free = svm_fit_rule.solve_batch(K, batch, SVM_SOLVE_EPS, 10_000_000)
    max_iter = int(np.median(free.n_iter))
    if nan:
        K = K.copy()
        a, b = np.flatnonzero(y == k - 2)[0], np.flatnonzero(y == k - 1)[0]
        K[a, b] = K[b, a] = np.nan
    return K, batch, max_iter


def _svm_solve_case(id, m, ld, k, seed, nan, big=None):
    K, batch, max_iter = svm_solve_batch(m, k, seed, nan)
    tab, rows, ev = batch.problems, batch.rows, batch.eval_rows
    Q = len(tab)

    def call(Lb, h, p, stream):
        from warpdemux_amd import _lib
        _lib.check(Lb.wdx_svm_solve_device(h, vp(p["d_K"]), m, ld, _lib.ptr(tab), Q, _lib.ptr(rows), len(rows), _lib.ptr(ev), len(ev), SVM_SOLVE_EPS,
                                           max_iter, vp(p["d_alpha"]), vp(p["d_rho"]), vp(p["d_n_iter"]), vp(p["d_state"]), vp(p["d_dec"]), stream))
        return {}

    def engine(eng, t):
        r = eng.svm_solve(t["d_K"], tab, rows, ev, eps=SVM_SOLVE_EPS, max_iter=max_iter)
        return dict(d_alpha=r.alpha, d_rho=r.rho, d_n_iter=r.n_iter, d_state=r.state, d_dec=r.dec)

    def rule():
        s = svm_fit_rule.solve_batch(K, batch, SVM_SOLVE_EPS, max_iter)
        return dict(d_alpha=s.alpha, d_rho=s.rho, d_n_iter=s.n_iter, d_state=s.state, d_dec=s.dec)

    c = Case(id, call, engine, rule, inputs=dict(d_K=pack(K, ld)),
             outputs=dict(d_alpha=(len(rows), "float64"), d_rho=(Q, "float64"), d_n_iter=(Q, "int64"), d_state=(Q, "int32"),
                          d_dec=(len(ev), "float64")), big=big)
    c.matrix = dict(d_K=(m, ld, m))
    return c


def svm_solve_cases():
    """m = 40, ld = 41, three classes: 3 full problems and their fold problems with evaluation rows; d_alpha exactly n_rows and d_dec
    exactly n_eval long; problems that end at max_iter (state 1) and problems with a NaN in their rows of K (state 2)"""
    return [_svm_solve_case("m40-ld41", SVM_SOLVE_M, SVM_SOLVE_LD, 3, 12, True, lambda: _svm_solve_case("big", 120, 120, 2, 5, False))]


def _distances(m, seed):
    rng = np.random.default_rng(seed)
    D = np.abs(rng.normal(0, 3.0, (m, m))).astype(np.float32)
    D[0, m - 1], D[m - 1, 0], D[m // 2, m // 3] = np.inf, np.nan, 0.0
    return D


def _svm_kernel_case(id, m, ld, ldk, off_d, off_k, inplace=False, pwr=2, gamma=0.05):
    D = _distances(m, 100 + m)
    want = lambda: pack(svm_cv_rule.kernel_matrix(D, gamma, pwr), ldk, pad=0)   # noqa: E731

    def call(Lb, h, p, stream):
        from warpdemux_amd import _lib
        _lib.check(Lb.wdx_svm_kernel_device(h, vp(p["d_D"]), m, ld, gamma, pwr, vp(p["d_D" if inplace else "d_K"]), ldk, stream))
        return {}

    def engine(eng, t):
        import torch
        full = t["d_D:full"] if inplace else torch.zeros((m, ldk), dtype=torch.float32, device="cuda")
        eng.svm_kernel(t["d_D"], gamma, pwr, out=t["d_D"] if inplace else full[:, :m])
        return {("d_D" if inplace else "d_K"): full}

    if inplace:
        c = Case(id, call, engine, lambda: dict(d_D=want()), inouts=dict(d_D=pack(D, ld)), written=dict(d_D=pack_mask(m, ld, m)),
                 offsets=dict(d_D=off_d))
    else:
        c = Case(id, call, engine, lambda: dict(d_K=want()), inputs=dict(d_D=pack(D, ld)), outputs=dict(d_K=((m - 1) * ldk + m, "float32")),
                 written=dict(d_K=pack_mask(m, ldk, m)), offsets=dict(d_D=off_d, d_K=off_k))
    c.matrix = dict(d_D=(m, ld, m))
    return c


def svm_kernel_cases():
    """m = 5 and m = 1 029 (a second run of 1 024 columns with a ragged end of 5); (ld, ldk) = (m, m), (round4, round4), (round4, m); the
    base pointers of D, of K and of both 4 bytes off a 16-byte boundary -- with ld and ldk multiples of four that is the branch only
    the base-pointer term of the `vec` decision keeps off the 16-byte accesses --; in place with both offsets.  Every case is the rule bit
    for bit, so the vector and the scalar paths give the same bits."""
    out = []
    for m in (5, SVM_KERNEL_COLS + SVM_KERNEL_VEC + 1):
        r4 = (m + 3) // 4 * 4
        for ld, ldk in ((m, m), (r4, r4), (r4, m)):
            for od, ok in ((0, 0), (4, 0), (0, 4), (4, 4)):
                out.append(_svm_kernel_case("m%d-ld%d-ldk%d-D%d-K%d" % (m, ld, ldk, od, ok), m, ld, ldk, od, ok))
        for ld in (m, r4):
            for od in (0, 4):
                out.append(_svm_kernel_case("m%d-ld%d-inplace-D%d" % (m, ld, od), m, ld, ld, od, od, inplace=True))
    return out


def couple_reference(dec, A, B, k):
    """(prob, stopping margin) of rows of decision values (n, pairs) in float64 NumPy: libsvm's sigmoid_predict, the clamp,
    multiclass_probability (tests/helpers/svm_ref.py) -- the reference tests/test_gpu_svm_cv.py holds the coupling kernel to"""
    fApB = dec * A[None, :] + B[None, :]
    with np.errstate(over="ignore"):
        e_neg, e_pos = np.exp(-fApB), np.exp(fApB)
        sig = np.where(fApB >= 0, e_neg / (1.0 + e_neg), 1.0 / (1.0 + e_pos))
    v = np.minimum(np.maximum(sig, svm_ref.MIN_PROB), 1 - svm_ref.MIN_PROB)
    r = np.zeros((len(dec), k, k))
    for q, (i, j) in enumerate(svm_ref._pairs(k)):
        r[:, i, j] = v[:, q]
        r[:, j, i] = 1 - v[:, q]
    prob, margin, _ = svm_ref._multiclass_probability(r)
    return prob, margin


COUPLE_ATOL, COUPLE_MARGIN = 1e-12, 1e-8   # tests/test_gpu_svm_cv.py: the bound of its exact tier and that tier's stopping margin


def _cv_couple_case(id, counts, k, seed, with_nan, big=None):
    rng = np.random.default_rng(seed)
    F, pairs, total = len(counts), k * (k - 1) // 2, int(sum(counts))
    m = total + 5                                                      # five rows no fold holds: they keep what they held
    held = rng.permutation(m)[:total].astype(np.int32)
    held_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    A, B = -rng.uniform(0.3, 4.0, (F, pairs)), rng.normal(0.0, 0.5, (F, pairs))
    off, at = np.zeros((F, pairs), np.int64), 2
    for c in rng.permutation(F * pairs):                               # every (fold, pair) block somewhere of its own, in shuffled order
        off[c // pairs, c % pairs] = at
        at += counts[c // pairs] + int(rng.integers(0, 3))
    n_dec = at                                                         # the last block may end on the last decision value
    dec = rng.normal(0.0, 1.5, n_dec)
    nan_rows = []
    if with_nan:
        f = int(np.flatnonzero(np.asarray(counts) > 0)[-1])
        e = counts[f] - 1
        dec[off[f, pairs - 1] + e] = np.nan
        nan_rows = [int(held[held_off[f] + e])]
    mask = np.zeros(m, bool)
    mask[held] = True

    def call(Lb, h, p, stream):
        from warpdemux_amd import _lib
        _lib.check(Lb.wdx_svm_cv_couple_device(h, vp(p["d_dec"]), n_dec, k, F, _lib.ptr(off), _lib.ptr(A), _lib.ptr(B), _lib.ptr(held), _lib.ptr(held_off),
                                               m, vp(p["d_prob"]), vp(p["d_pred_idx"]), vp(p["d_conf"]), stream))
        return {}

    def engine(eng, t):
        import torch
        o = dict(d_prob=torch.zeros(m * k, dtype=torch.float64, device="cuda"), d_pred_idx=torch.zeros(m, dtype=torch.int32, device="cuda"),
                 d_conf=torch.zeros(m, dtype=torch.float64, device="cuda"))
        call(eng.L, eng.ctx.handle, dict(d_dec=t["d_dec"].data_ptr(), **{n: v.data_ptr() for n, v in o.items()}), eng._stream())
        return o

    def reference_rows():
        """how many held-out rows the probability bound is applied to: those beyond the reference's stopping margin"""
        used = 0
        for f in range(F):
            if counts[f]:
                rows = np.stack([dec[off[f, q]:off[f, q] + counts[f]] for q in range(pairs)], axis=1)
                used += int((couple_reference(rows[~np.isnan(rows).any(axis=1)], A[f], B[f], k)[1] >= COUPLE_MARGIN).sum())
        return used

    def check(got):
        prob, pred, conf = got["d_prob"].reshape(m, k), got["d_pred_idx"], got["d_conf"]
        assert reference_rows() > 0, "%s: no row beyond the stopping margin: the probability bound would hold nothing" % id
        for f in range(F):
            H = held[held_off[f]:held_off[f + 1]]
            if not len(H):
                continue
            rows = np.stack([dec[off[f, q]:off[f, q] + counts[f]] for q in range(pairs)], axis=1)
            ok = ~np.isnan(rows).any(axis=1)
            want, margin = couple_reference(rows[ok], A[f], B[f], k)
            use = margin >= COUPLE_MARGIN
            err = np.abs(prob[H[ok]][use] - want[use]).max(initial=0.0)
            assert err <= COUPLE_ATOL, "%s fold %d: probabilities %.3g from couple_reference (bound %.0e)" % (id, f, err, COUPLE_ATOL)
            own = np.sort(prob[H[ok]], axis=1)
            assert np.array_equal(pred[H[ok]], np.argmax(prob[H[ok]], axis=1)) and np.array_equal(conf[H[ok]], own[:, -1] - own[:, -2]), \
                "%s fold %d: the index or the margin is not that of the row's own probabilities" % (id, f)
        for r in nan_rows:
            assert np.isnan(prob[r]).all() and pred[r] == -1 and np.isnan(conf[r]), "%s: row %d has a NaN decision value" % (id, r)

    c = Case(id, call, engine, None, inputs=dict(d_dec=dec), check=check,
             outputs=dict(d_prob=(m * k, "float64"), d_pred_idx=(m, "int32"), d_conf=(m, "float64")),
             written=dict(d_prob=np.repeat(mask, k), d_pred_idx=mask, d_conf=mask), big=big)
    c.reference_rows, c.finite_rows = reference_rows, total - len(nan_rows)
    return c


def cv_couple_cases():
    """1, 5, 6 and 7 held-out rows (3, 3, 2 and 1 idle groups behind the last row of a wave of four); k = 2, 7 (21 pairs: a second trip
    of the gather loop) and 16; 3 folds, one empty in the middle -- and, in the second layout, one empty at the end as well --; five rows
    no fold holds; one NaN decision value from 5 rows on; the (fold, pair) blocks in shuffled order"""
    big = lambda: _cv_couple_case("big", (61, 60, 60, 60, 59), 10, 77, False)   # noqa: E731
    out = []
    for total in (1, CV_ROWS_PER_WAVE + 1, CV_ROWS_PER_WAVE + 2, CV_ROWS_PER_WAVE + 3):
        for k in CV_CLASSES:
            layouts = [("end", (total, 0, 0))] + ([("mid", (total - total // 2, 0, total // 2))] if total > 1 else [])
            for name, counts in layouts:
                out.append(_cv_couple_case("rows%d-k%d-%s" % (total, k, name), counts, k, 31 * total + k, total >= 5, big))
    return out


def _thresholds_case(id, n, k, R, T, seed, big=None, null_big=True):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, k, n).astype(np.int32)
    logits = rng.normal(size=(n, k)) + 2.0 * (np.arange(k)[None, :] == y[:, None])
    e = np.exp(logits - logits.max(axis=1, keepdims=True)) if n else logits
    prob = np.ascontiguousarray(e / e.sum(axis=1, keepdims=True)) if n else np.zeros((0, k))
    prob[::7] = np.round(prob[::7], 2)          # margins that sit on or next to grid values
    if n >= 20:
        y[rng.random(n) < 0.2] = 0
        y[3], y[9] = -1, k                      # skipped | used, and no prediction hits it
        prob[5, 1] = np.nan
    pm = np.array([990], np.int32) if T == 1 else np.linspace(0, 1000, T).round().astype(np.int32)
    bins = R + 1

    def call(Lb, h, p, stream):
        from warpdemux_amd import _lib
        _lib.check(Lb.wdx_accuracy_thresholds_device(h, vp(p["d_prob"]), n, k, vp(p["d_y_idx"]), R, _lib.ptr(pm), T, vp(p["d_thr"]), vp(p["d_kept"]),
                                                     vp(p["d_hit"]), vp(p["d_skipped"]), stream))
        return {}

    def engine(eng, t):
        thr, kept, hit, skipped = eng.accuracy_thresholds(t["d_prob"].view(n, k), t["d_y_idx"], tuple(float(v) / 1000.0 for v in pm), R)
        return dict(d_thr=thr, d_kept=kept, d_hit=hit, d_skipped=skipped)

    def rule():
        thr, kept, hit, skipped = svm_cv_rule.thresholds_brute(prob, y, pm, R)
        return dict(d_thr=_flat(thr), d_kept=_flat(kept), d_hit=_flat(hit), d_skipped=np.array([skipped], np.int64))

    return Case(id, call, engine, rule, inputs=dict(d_prob=_flat(prob), d_y_idx=y),
                outputs=dict(d_thr=(T * k, "float64"), d_kept=(k * bins, "int64"), d_hit=(k * bins, "int64"), d_skipped=(1, "int64")),
                nullable=("d_kept", "d_hit", "d_skipped"), big=big, null_big=null_big)


def thresholds_cases():
    """n = 0, 1 and one row either side of the 4 096 rows of a histogram workgroup; k = 2 and 16, at R = 400 in two class groups;
    R = 1, 63, 64, 65 (the select kernel walks 64 bins a step); 1 and 16 targets; rows with y_idx < 0, y_idx >= k and a NaN probability;
    the histograms given and NULL -- the NULL form also right behind a call with k = 16 and R = 500 on the context's own histograms"""
    big = lambda: _thresholds_case("big", 3 * THR_ROWS, 16, 500, 3, 9)   # noqa: E731
    B = THR_SELECT_BINS
    shapes = [(0, 2, 1, 1), (1, 2, 1, 1), (1, 16, B, 16), (THR_ROWS - 1, 2, B - 1, 1), (THR_ROWS, 16, B + 1, 16), (THR_ROWS + 1, 16, B, 1),
              (THR_ROWS + 1, 2, B + 1, 16), (300, 16, THR_LDS_ENTRIES // 32 + 16, 16), (200, 16, B - 1, 1), (200, 2, 1, 16),
              (500, 2, 3 * B + 8, 16)]
    return [_thresholds_case("n%d-k%d-R%d-T%d" % s, *s, seed=sum(s), big=big) for s in shapes]


# ---- the trainers -----------------------------------------------------------------------------------------------------------------------

def _mlp_case(id, m, F, ld, hidden, k, batch, with_order, seed, epochs=2, big=None):
    from warpdemux_amd import _mlp_fit
    rng = np.random.default_rng(seed)
    y = (np.arange(m) % k).astype(np.int32)
    rng.shuffle(y)
    D = np.abs(rng.normal(size=(k, F))[y] * 3.0 + rng.normal(size=(m, F))).astype(np.float32)
    mean, scale = D.astype(np.float64).mean(axis=0), D.astype(np.float64).std(axis=0) + 1e-3
    sizes = _mlp_fit.layer_sizes(F, [hidden], k)
    W0, B0, order = _mlp_fit.schedule(sizes, "relu", seed, m, epochs, shuffle=with_order)
    kw = dict(lr=1e-2, alpha=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-8, tol=1e-4)

    def host(fit):
        out = {"coefs%d" % i: w for i, w in enumerate(fit.coefs)}
        out.update({"intercepts%d" % i: b for i, b in enumerate(fit.intercepts)})
        out.update(loss_curve=fit.loss_curve, n_epochs=np.array([fit.n_iter]), state=np.array([fit.state]))
        return out

    def call(Lb, h, p, stream):
        P = _mlp_fit.params_c(sizes, "relu", k, batch, epochs, 10, *kw.values())
        W, B, mu, sc, od = _mlp_fit.check_arrays(sizes, m, W0, B0, mean, scale, order, epochs)
        return host(_mlp_fit.call(Lb.wdx_mlp_fit_device, h, vp(p["d_dist"]), m, ld, vp(p["d_y"]), P, W, B, mu, sc, od, stream=stream))

    def engine(eng, t):
        return host(eng.mlp_fit(t["d_dist"], t["d_y"], W0, B0, activation="relu", n_classes=k, mean=mean, scale=scale, order=order,
                                batch_size=batch, max_epochs=epochs, n_iter_no_change=10, learning_rate_init=kw["lr"], alpha=kw["alpha"],
                                beta_1=kw["beta1"], beta_2=kw["beta2"], epsilon=kw["epsilon"], tol=kw["tol"]))

    c = Case(id, call, engine, None, inputs=dict(d_dist=pack(D, ld), d_y=y), big=big)
    c.matrix = dict(d_dist=(m, ld, F))
    return c


def mlp_fit_cases():
    """m = 17 rows (a workgroup takes 16), ld = 18; 17 -> 17 -> 3 and 17 -> 5 -> 1 (two classes); batches of 16 and of 5; 2 epochs; an explicit
    order and NULL"""
    big = lambda: _mlp_case("big", 60, 60, 60, 32, 4, 25, True, 3)   # noqa: E731
    m = MLP_FIT_ROWS + 1
    return [_mlp_case("h%d-k%d-b%d-%s" % (h, k, b, "order" if o else "no-order"), m, m, m + 1, h, k, b, o, 40 + h + b, big=big)
            for h, k in ((17, 3), (5, 2)) for b in (MLP_FIT_ROWS, 5) for o in (True, False)]


BOOST_LR, BOOST_LAM = 0.3, 3.0


def _boost_case(id, n, F, ld, k, depth, seed, n_trees=2, big=None):
    from warpdemux_amd import _boost_fit
    X, y = boost_fit_rule.synthetic(n, F, k, seed)
    y = y.astype(np.int32)
    X[:, 1] = 0.25                                                     # one value: the feature has no border
    if n > 20:
        X[7, 0] = np.nan
        borders = _boost_fit.borders(X, 8)
    else:
        borders = [np.array([-0.5, 0.5], np.float32), np.zeros(0, np.float32)] + [np.array([0.0], np.float32)] * (F - 2)
    assert len(borders[1]) == 0
    flat, nb = _boost_fit.pack_borders(borders)
    B = max(1, int(nb.max()))

    def host(fits):
        return {"%s%d" % (name, i): getattr(f, name) for i, f in enumerate(fits) for name in ("split_feature", "split_border", "leaf_values")}

    def call(Lb, h, p, stream):
        P = _boost_fit.params_c(F, k, n_trees, depth, B, BOOST_LR, BOOST_LAM)
        return host([_boost_fit.call(Lb.wdx_boost_fit_device, h, vp(p["d_X"]), n, ld, vp(p["d_y"]), flat, nb, P, vp(p["d_scores"]), stream=stream)
                     for _ in range(2)])                               # the second call continues the fit

    def engine(eng, t):
        S = t["d_scores"].view(n, k)
        fits = [eng.boost_fit(t["d_X"], t["d_y"], borders, S, n_trees=n_trees, depth=depth, learning_rate=BOOST_LR, l2_leaf_reg=BOOST_LAM,
                              border_count=B) for _ in range(2)]
        return dict(d_scores=S, **host(fits))

    def rule():
        out, S = {}, None
        for i in range(2):
            fit, S = boost_fit_rule.fit(X, y, k, n_trees, depth, BOOST_LR, BOOST_LAM, B, scores=S, border_list=borders)
            out.update({"split_feature%d" % i: np.array(fit.split_feature, np.int32), "split_border%d" % i: np.array(fit.split_border, np.int32),
                        "leaf_values%d" % i: np.array(fit.leaf_values)})
        out["d_scores"] = _flat(S)
        return out

    c = Case(id, call, engine, rule, inputs=dict(d_X=pack(X, ld), d_y=y), inouts=dict(d_scores=np.zeros(n * k)), big=big)
    c.matrix = dict(d_X=(n, ld, F))
    return c


def boost_fit_cases():
    """n = 1 and n = 2 048 (one row more than a histogram pass takes); 3 features, one of them without borders; ld = 4; k = 2 and 3; depth 1
    and 2; 2 trees, and 2 more from a second call on the in/out scores, which lie in an exact frame"""
    big = lambda: _boost_case("big", 3 * BOOST_FIT_ROWS, 6, 6, 4, 3, 21)   # noqa: E731
    return [_boost_case("n%d-k%d-depth%d" % (n, k, d), n, 3, 4, k, d, 50 + k + d, big=big) for n in (1, BOOST_FIT_ROWS + 1) for k in (2, 3)
            for d in (1, 2)]


# ---- the table ------------------------------------------------------------------------------------------------------------------------------

_STATUS = Arg("d_status", IN_NULLABLE, "int32[n]")

ENTRIES = {e.name: e for e in (
    Entry("wdx_medoids_device",
          (Arg("dX", IN, "float64 (n, L)"), Arg("label", HOST, "int32[n]"), _STATUS, Arg("d_medoid", OUT, "int64[n_labels]"),
           Arg("d_medoid_cost", OUT_NULLABLE, "float64[n_labels]"), Arg("d_count", OUT_NULLABLE, "int64[n_labels]"),
           Arg("d_cost", OUT_NULLABLE, "float64[n]"), Arg("d_refs", OUT_NULLABLE, "float64 (n_labels, L)")),
          "medoids", "medoid_rule.medoid_rule", medoid_cases),
    Entry("wdx_self_matrix_device",
          (Arg("dX", IN, "float64 (n, L)"), _STATUS, Arg("d_out", OUT, "float32, (n-1) ld + n elements; columns n .. ld-1 not written")),
          "self_distances", "self_matrix_rule.self_matrix_rule", self_matrix_cases),
    Entry("wdx_self_nearest_device",
          (Arg("dX", IN, "float64 (n, L)"), Arg("d_label", IN_NULLABLE, "int32[n]"), _STATUS, Arg("d_nn", OUT, "int32 (n, 2)"),
           Arg("d_best", OUT, "float32 (n, 2)")),
          "loo_nearest", "loo_rule.loo_rule", self_nearest_cases),
    Entry("wdx_dba_step_device",
          (Arg("dX", IN, "float64 (n, L)"), Arg("label", HOST, "int32[n]"), _STATUS, Arg("d_centres", IN, "float64 (n_labels, L)"),
           Arg("d_new", OUT, "float64 (n_labels, L)"), Arg("d_count", OUT_NULLABLE, "int64[n_labels]"),
           Arg("d_inertia", OUT_NULLABLE, "float64[n_labels]"), Arg("d_cost", OUT_NULLABLE, "float64[n]"),
           Arg("d_runs", OUT_NULLABLE, "int32 (n, L, 2)")),
          "dba_step", "dba_rule.dba_step", dba_cases),
    Entry("wdx_svm_solve_device",
          (Arg("d_K", IN, "float32, (m-1) ld + m elements"), Arg("problems", HOST, "wdx_svm_problem[n_problems]"), Arg("rows", HOST, "int32[n_rows]"),
           Arg("eval_rows", HOST, "int32[n_eval]"), Arg("d_alpha", OUT, "float64[n_rows]"), Arg("d_rho", OUT, "float64[n_problems]"),
           Arg("d_n_iter", OUT, "int64[n_problems]"), Arg("d_state", OUT, "int32[n_problems]"), Arg("d_dec", OUT, "float64[n_eval]")),
          "svm_solve", "svm_fit_rule.solve_batch", svm_solve_cases),
    Entry("wdx_svm_kernel_device",
          (Arg("d_D", IN, "float32, (m-1) ld + m elements"), Arg("d_K", OUT, "float32, (m-1) ldk + m elements; columns from m on not written")),
          "svm_kernel", "svm_cv_rule.kernel_matrix", svm_kernel_cases),
    Entry("wdx_svm_cv_couple_device",
          (Arg("d_dec", IN, "float64[n_dec]"), Arg("dec_off", HOST, "int64[n_folds * pairs]"), Arg("probA", HOST, "float64[n_folds * pairs]"),
           Arg("probB", HOST, "float64[n_folds * pairs]"), Arg("held", HOST, "int32[total]"), Arg("held_off", HOST, "int64[n_folds + 1]"),
           Arg("d_prob", OUT, "float64 (m, k); a row no fold holds not written"), Arg("d_pred_idx", OUT, "int32[m]; likewise"),
           Arg("d_conf", OUT, "float64[m]; likewise")),
          "svm_cross_val",
          "no bit-for-bit NumPy rule exists (the coupling iterates to a stopping margin): device_entries.couple_reference at the bound of "
          "tests/test_gpu_svm_cv.py, and the index and the margin exactly from the device's own probabilities",
          cv_couple_cases,
          second="ctypes"),   # svm_cross_val runs the whole cross-validation (plan, solve, sigmoid fits) in front of this call
    Entry("wdx_accuracy_thresholds_device",
          (Arg("d_prob", IN, "float64 (n, k)"), Arg("d_y_idx", IN, "int32[n]"), Arg("targets_pm", HOST, "int32[n_targets]"),
           Arg("d_thr", OUT, "float64 (n_targets, k)"), Arg("d_kept", OUT_NULLABLE, "int64 (k, R + 1)"), Arg("d_hit", OUT_NULLABLE, "int64 (k, R + 1)"),
           Arg("d_skipped", OUT_NULLABLE, "int64[1]")),
          "accuracy_thresholds", "svm_cv_rule.thresholds_brute", thresholds_cases),
    Entry("wdx_mlp_fit_device",
          (Arg("d_dist", IN, "float32, (m-1) ld + sizes[0] elements"), Arg("d_y", IN, "int32[m]"), Arg("p", HOST, "wdx_mlp_fit_params"),
           Arg("mean", HOST, "float64[sizes[0]]"), Arg("scale", HOST, "float64[sizes[0]]"), Arg("coefs", HOST_OUT, "float32 (sizes[l], sizes[l+1]) per layer"),
           Arg("intercepts", HOST_OUT, "float32[sizes[l+1]] per layer"), Arg("order", HOST, "int32 (max_epochs, m)"),
           Arg("loss_curve", HOST_OUT, "float64[max_epochs]"), Arg("n_epochs", HOST_OUT, "int32"), Arg("state", HOST_OUT, "int32")),
          "mlp_fit", "none here: helpers/mlp_fit_rule.py is float64, its accuracy bound stays in tests/test_gpu_mlp_fit.py", mlp_fit_cases),
    Entry("wdx_boost_fit_device",
          (Arg("d_X", IN, "float64, (n-1) ld + n_features elements"), Arg("d_y", IN, "int32[n]"), Arg("borders", HOST, "float32[sum(n_borders)]"),
           Arg("n_borders", HOST, "int32[n_features]"), Arg("p", HOST, "wdx_boost_fit_params"), Arg("d_scores", INOUT, "float64 (n, k)"),
           Arg("split_feature", HOST_OUT, "int32[n_trees * depth]"), Arg("split_border", HOST_OUT, "int32[n_trees * depth]"),
           Arg("leaf_values", HOST_OUT, "float64[n_trees * 2^depth * k]")),
          "boost_fit", "boost_fit_rule.fit", boost_fit_cases),
)}


# ---- the stream contract: where each row's late-input case is ------------------------------------------------------------------------------
LATE_HERE = {"wdx_svm_cv_couple_device": ("rows7-k7-mid", False), "wdx_accuracy_thresholds_device": ("n4097-k16-R64-T1", False),
             "wdx_mlp_fit_device": ("h17-k3-b5-order", True), "wdx_boost_fit_device": ("n2048-k3-depth2", True)}   # entry -> (case, blocks by contract)
LATE_ELSEWHERE = {"wdx_medoids_device": "test_gpu_medoids.py", "wdx_self_matrix_device": "test_gpu_self_matrix.py",
                  "wdx_self_nearest_device": "test_gpu_loo.py", "wdx_dba_step_device": "test_gpu_dba.py",
                  "wdx_svm_solve_device": "test_gpu_svm_fit.py", "wdx_svm_kernel_device": "test_gpu_svm_kernel.py"}
THR_WS_PAIR = ("n4096-k16-R65-T16", "n500-k2-R200-T16")   # the context's own histograms at one (k, R), then at another


@functools.lru_cache(maxsize=None)
def cases(name):
    return tuple(ENTRIES[name].cases())


def case(name, id):
    return next(c for c in cases(name) if c.id == id)


def case_ids():
    """[(entry, case id)] of the whole table, in the table's order"""
    return [(name, c.id) for name in ENTRIES for c in cases(name)]
