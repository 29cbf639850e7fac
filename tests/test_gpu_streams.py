"""The stream contract of the device-resident entry points (include/wdx.h): "enqueued on `stream`; no synchronisation", "the
workspaces of a context are ordered by stream order; when consecutive calls name different streams the library waits for the
earlier stream first", and "a resident reference set or model is not replaced under work that is still reading it".

Every other GPU test calls the device entries on torch's default stream -- the legacy NULL stream, which orders itself against
everything -- so a launch, copy or memset put on the wrong stream, or a shared buffer reused too early, is invisible there.
Here every call runs on a torch SIDE stream (hipStreamNonBlocking) whose inputs arrive LATE: the tensors hold a decoy (another
valid batch) until, behind a device-side delay on that stream, the real values are copied in.  A call that did not honour the
stream computes the decoy's results -- wrong values, never a fault.

  (A) one side stream, late inputs: every `DemuxEngine` device method returns the serial result, and (asynchrony) an event
      recorded right behind the delay is still pending when the call returns
  (B) two streams on one context, one shared buffer per case: call 1 on the delayed stream, call 2 at once on the other; both
      equal their serial results, and work enqueued behind call 2 sees what the delayed stream wrote (the library did wait)
  (C) the resident reference set / model replaced behind pending work: call 1 keeps the old state, call 2 gets the new one
  (D) wdx_ctx_synchronize(ctx, A): a copy made on B afterwards sees finished results
  (E) a minibatch in flight (wdx_demux_submit_ex) keeps the reference set and the models it was submitted with (the SVM and the
      boost model: the minibatch path has no WDX_WANT bit for the MLP tail, so no slot ever reads that model, and
      wdx_mlp_set_model is held by (C) alone; the three model setters wait in one shared function, wdx_classify.hip: install)

The reference of every comparison is the same call made serially on a SECOND context on the default stream, bit for bit; the
plain fingerprint + DTW case of (A) is compared with the CPU oracle as well.  Each test body runs in a fresh child process
(this file with arguments; tests/helpers/stream_order.py: `run_child`), which first proves that its two side streams overtake
one another (`side_streams`): without that control the ordering assertions would pass vacuously, so a child without such a
pair FAILS.  No test synchronises the device or the context between enqueuing and reading back ((D) is about that call).
"""
import ctypes as C
import functools
import json
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.abspath(__file__)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import stream_order as so  # noqa: E402

pytestmark = pytest.mark.gpu

K, N_REFS, WINDOW, PENALTY = 25, 6, 15, 0.1
STRIDE = 6208                     # rows of tests/helpers/refine_inputs.py (at most 6 200 samples), a multiple of 8
LONG = 16704                      # the row of a read with a window of 16 600 samples
SMALL, LARGE = 300, 8200          # read-minor DTW copy and context buffers | row-major DTW, launch slices of 3 000
LAUNCH_SLICE = 3000               # OPT_MAX_LAUNCH_SLICE of the engines with LARGE batches
OPTIMAL_LARGE = 800               # reads of the optimal change-points variants when the batch is LARGE (child_A says why)

A_GROUPS = ("fingerprint", "demux", "nearest", "tails", "adc")
B_CASES = ("fp_ws", "ref_buf", "ref_buf_optimal", "fp_big", "fp_long", "adc_stage", "dtw", "dtw_wavefront", "dtw_wide",
           "nearest_buf", "svm_host_dtw", "engine_work", "timed")
C_CASES = ("refs", "svm", "mlp", "boost")
E_CASES = ("refs", "boost", "svm")


# ---- the tests: one child each ------------------------------------------------------------------------------------------------

def _child(*args, timeout=150.0):
    res, _ = so.run_child(HERE, args, timeout=timeout)
    assert res.get("ok") is True, res
    return res


@pytest.mark.parametrize("n", [SMALL, LARGE])
@pytest.mark.parametrize("group", A_GROUPS)
def test_late_inputs_on_one_side_stream(group, n):
    """(A): every device method of the group on side stream A with late inputs equals the serial call, and returns while the
    delay in front of its inputs is still running"""
    res = _child("A", group, n)
    assert res["checked"] and all(c["same"] and (c["pending"] or c["exempt"]) for c in res["checked"]), res


@pytest.mark.parametrize("case", B_CASES)
def test_two_streams_share_one_context(case):
    """(B): call 1 behind the delay on one stream, call 2 at once on the other, then the roles swapped"""
    res = _child("B", case)
    assert len(res["checked"]) == 2 and all(c["same"] and c["ordered"] for c in res["checked"]), res


@pytest.mark.parametrize("case", C_CASES)
def test_resident_state_replaced_behind_pending_work(case):
    """(C): the replacement (same sizes: nothing is reallocated) waits for the call that still reads the old state"""
    res = _child("C", case)
    assert len(res["checked"]) == 2 and all(c["same"] for c in res["checked"]), res


def test_ctx_synchronize_names_a_callers_stream():
    """(D): test_ctx_synchronize_null_names_the_null_stream_and_the_context_stream, for a caller's stream"""
    _child("D")


@pytest.mark.parametrize("case", E_CASES)
def test_minibatch_in_flight_keeps_what_it_was_submitted_with(case):
    """(E): wdx_set_refs / wdx_boost_set_model / wdx_svm_set_model at once behind wdx_demux_submit_ex on a page-locked minibatch
    of 2 048 x 8 192 samples; the batch carries the results of the state at submit, a second batch those of the new state.
    Vacuous (and failed) unless the batch is in flight for more than 20 x the setter's own host time."""
    res = _child("E", case)
    assert res["first_same"] and res["second_same"] and res["states_differ"], res
    assert res["flight_s"] > 20.0 * res["setter_s"], ("vacuous: the batch was not in flight long enough", res)


# ==== from here on: the child process ===========================================================================================

def _imports():
    global torch, _lib, models, sig_proc, DemuxEngine, AdcShard, ri, li, dtw_cases, svm_ref, mlp_ref, boost_ref, orc
    import torch
    from helpers import boost_ref, dtw_cases, mlp_ref, svm_ref
    from helpers import long_inputs as li
    from helpers import refine_inputs as ri
    from oracle import wdx_oracle as orc
    from warpdemux_amd import _lib, models, sig_proc
    from warpdemux_amd.engine import AdcShard, DemuxEngine


def _np(x):
    return None if x is None else (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 2: np.int16, 1: np.uint8}[a.dtype.itemsize])


def _same(got, want):
    """every output bit for bit (None stays None)"""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if g is None or w is None:
            if g is not w:
                return False
            continue
        if g.dtype != w.dtype or g.shape != w.shape or not np.array_equal(_bits(g), _bits(w)):
            return False
    return True


def _read_back(outs):
    """.cpu() of every output under the CURRENT stream (the one that produced them)"""
    return [_np(o) for o in outs]


class Inputs:
    """The device tensors of one call (`t`, by name) with their real values and a decoy in device staging."""

    def __init__(self, real, decoy=None):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        self.real = {k: dev(v) for k, v in real.items()}
        # the decoy: the same reads 37 places further on -- a valid batch of the same shapes and window lengths
        self.decoy = {k: (dev(decoy[k]) if decoy is not None else v.roll(37, 0)) for k, v in self.real.items()}
        self.t = {k: v.clone() for k, v in self.real.items()}
        torch.cuda.synchronize()

    def _seq(self, d):
        return [d[k] for k in self.t]

    def late(self, stream, ms):
        return so.late(stream, self._seq(self.t), self._seq(self.real), self._seq(self.decoy), ms)

    def fill(self, which):
        for k, v in self.t.items():
            v.copy_(getattr(self, which)[k])
        torch.cuda.synchronize()


def _serial(eng, op, inp, which="real"):
    """the reference: the call made serially on the default stream, the device synchronised before and after"""
    torch.cuda.synchronize()
    out = _read_back(op(eng, getattr(inp, which)))
    torch.cuda.synchronize()
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

def _reads(n, seed, long_at=()):
    """n reads of tests/helpers/refine_inputs.py (its 96, then draws of them) in rows of STRIDE samples with NaN tails, and at
    the places `long_at` a read whose adapter window has 16 600 samples: beyond WDX_MAX_ADAPTER_SAMPLES, status 5."""
    b = _batch(seed)
    idx = np.concatenate([np.arange(96), np.random.default_rng(seed).integers(0, 96, max(n - 96, 0))])[:n]
    w = b["rows"].shape[1]
    base = np.full((96, STRIDE), np.nan, dtype=np.float32)
    base[:, :w] = b["rows"]
    long_row = np.full(LONG, np.nan, dtype=np.float32)
    long_row[:16600] = li.step_row(np.random.default_rng(100 + seed), 16600)
    is_long = np.zeros(n, dtype=bool)
    is_long[list(long_at)] = True
    a_s, a_e, ok = b["a_s"][idx].copy(), b["a_e"][idx].copy(), b["ok"][idx].copy()
    a_s[is_long], a_e[is_long], ok[is_long] = ri.PADDING, 16600 - ri.PADDING, 1
    return dict(b=b, idx=idx, base=base, long_row=long_row, is_long=is_long, a_s=a_s, a_e=a_e, ok=ok)


def _packed(rd, shift=0):
    """the float32 reads as a packed device call takes them -- sig 1-D, off int64 (n + 1), a_s, a_e, ok -- every read `shift`
    places further on (the decoy of a batch: the same reads in another order, a valid batch of the same total size)"""
    n = len(rd["idx"])
    order = np.roll(np.arange(n), shift)
    is_long = rd["is_long"][order]
    off = np.concatenate([[0], np.cumsum(np.where(is_long, LONG, STRIDE))]).astype(np.int64)
    sig = np.empty(int(off[-1]), dtype=np.float32)
    cuts = [-1, *np.flatnonzero(is_long).tolist(), n]
    for r in cuts[1:-1]:
        sig[off[r]:off[r + 1]] = rd["long_row"]
    for r0, r1 in zip(cuts[:-1], cuts[1:]):             # the runs of ordinary reads between the long ones
        if r1 > r0 + 1:
            sig[off[r0 + 1]:off[r1]].reshape(-1, STRIDE)[:] = rd["base"][rd["idx"][order[r0 + 1:r1]]]
    return dict(sig=sig, off=off, a_s=rd["a_s"][order], a_e=rd["a_e"][order], ok=rd["ok"][order])


def _row_inputs(rd):
    return Inputs(_packed(rd), _packed(rd, 37))


def _shard_arrays(rd):
    """the int16 form of the reads, strided (a batch without long reads)"""
    assert not rd["is_long"].any()
    b, idx = rd["b"], rd["idx"]
    adc = np.full((len(idx), STRIDE), 12345, dtype=np.int16)
    adc[:, :b["adc"].shape[1]] = b["adc"][idx]
    return dict(adc=adc, row_len=b["row_len"][idx], offset=b["offset"][idx], scale=b["scale"][idx], a_s=rd["a_s"], a_e=rd["a_e"],
                ok=rd["ok"])


def _windows(rd):
    limit = np.where(rd["is_long"], LONG, STRIDE)
    return np.minimum(rd["a_e"].astype(np.int64) + ri.PADDING, limit) - np.maximum(rd["a_s"].astype(np.int64) - ri.PADDING, 0)


def _max_len(rd):
    """the longest adapter window of the batch, as a caller states it"""
    return int(_windows(rd)[rd["ok"] != 0].max())


def _seg():
    return sig_proc.SegParams(barcode_num_events=K, **ri.SEG)


@functools.lru_cache(maxsize=None)
def _batch(seed):
    return ri.batch(seed)


@functools.lru_cache(maxsize=None)
def _refs(seed=1):
    """N_REFS fingerprints of the reads themselves (the CPU oracle's), a little off"""
    b = _batch(seed)
    fpt, _, _, status = orc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], orc.SegParams(barcode_num_events=K, **ri.SEG), b["ok"])
    refs = np.ascontiguousarray(fpt[status == 0][:N_REFS]) + 0.01
    assert refs.shape == (N_REFS, K)
    return refs


def _svm(refs, seed):
    return svm_ref.synth_model(3, seed=seed, n_support=[2, 1, 3], n_extra=0, thresholds=True, gamma=0.02).to_dtw_svm(refs)


def _mlp(refs, seed):
    est = mlp_ref.random_mlp(len(refs), (16,), 5, np.float32, "relu", seed=seed)
    return models.from_reference(mlp_ref.DTW_MLP(est, refs, {i: 3 * i + 1 for i in range(5)}, np.linspace(0.05, 0.3, 5),
                                                 window=WINDOW, penalty=PENALTY))


def _boost(seed):
    bm = boost_ref.random_model(33, (0, 1, 6, 3), 4, K, seed=seed)
    trees = [(f, bo, [bm.nan_treatment[i] == "AsTrue" for i in f], lv) for f, bo, lv in bm.trees]
    return models.Fpt_Boost(trees, bm.n_features, bm.scale, bm.bias, {i: 2 * i + 1 for i in range(4)}, np.array([0.05, 0.2, 0.1, 0.3]))


def _engine(refs=None, large=False, with_models=True, params=None, window=WINDOW, **kw):
    refs = _refs() if refs is None else refs
    eng = DemuxEngine(refs, window, PENALTY, params or _seg(), **kw)
    if large:
        eng.ctx.set_option(_lib.OPT_MAX_LAUNCH_SLICE, LAUNCH_SLICE)
    if with_models:
        eng.set_svm(_svm(refs, 5))
        eng.set_mlp(_mlp(refs, 9))
        eng.set_boost(_boost(81))
    return eng


def _hr(qscale=1.0, optimal=False):
    return sig_proc.RefineParams(query=ri.consensus() * qscale, optimal_cpts=optimal, **ri.REF)


# ---- the calls: op(engine, tensors by name) -> tuple of output tensors ----------------------------------------------------------

def _rows_kw(t, max_len):
    return dict(ok=t["ok"], offsets=t["off"], max_len=max_len)


def op_fingerprint(ml):
    return lambda e, t: e.fingerprint(t["sig"], t["a_s"], t["a_e"], **_rows_kw(t, ml))


def op_fingerprint_refine(ml, hr):
    return lambda e, t: e.fingerprint_refine(t["sig"], t["a_s"], t["a_e"], hr, **_rows_kw(t, ml))


def _demux_out(r):
    return (r.dist, r.call, r.status, r.counts, r.fpt)


def op_demux(ml):
    return lambda e, t: _demux_out(e.demux(t["sig"], t["a_s"], t["a_e"], want_fpt=True, **_rows_kw(t, ml)))


def op_demux_refine(ml, hr):
    def op(e, t):
        r, dwell, stats, idx = e.demux_refine(t["sig"], t["a_s"], t["a_e"], hr, **_rows_kw(t, ml))
        return (*_demux_out(r), dwell, stats, idx)
    return op


def op_dtw(e, t):
    return e.dtw(t["X"])


def _rule(e):
    """device tensors of the nearest-reference rule (host arrays would be uploaded inside the call): two references per label"""
    lab = torch.arange(e.nY, dtype=torch.int32, device=e.tdev) // 2
    G = (e.nY + 1) // 2
    mm = torch.linspace(0.0, 0.5, G, dtype=torch.float32, device=e.tdev)
    md = torch.linspace(60.0, 20.0, G, dtype=torch.float32, device=e.tdev)
    return dict(labels=lab, n_labels=G, min_margin=mm, max_dist=md)


def op_nearest(want_dist, rule):
    def op(e, t):
        r = e.nearest(t["X"], want_dist=want_dist, status=t.get("st"), **rule)
        return (r.call, r.best, r.counts, r.dist)
    return op


def op_demux_nearest(ml, rule):
    def op(e, t):
        r = e.demux_nearest(t["sig"], t["a_s"], t["a_e"], want_dist=True, want_fpt=True, **rule, **_rows_kw(t, ml))
        return (r.call, r.best, r.status, r.counts, r.dist, r.fpt)
    return op


def op_demux_tail(kind, ml, want_dist=True, shard=False):
    def op(e, t):
        sig, kw = (_shard(t), dict(ok=t["ok"], max_len=ml)) if shard else (t["sig"], _rows_kw(t, ml))
        if kind == "boost":
            return e.demux_boost(sig, t["a_s"], t["a_e"], None, want_fpt=True, want_raw=True, **kw)
        if kind == "boost_refine":
            return e.demux_boost(sig, t["a_s"], t["a_e"], _hr(), want_fpt=True, want_raw=True, **kw)
        return getattr(e, "demux_" + kind)(sig, t["a_s"], t["a_e"], want_dist=want_dist, want_fpt=True, **kw)
    return op


def _shard(t):
    return AdcShard(t["adc"], t["row_len"], t["offset"], t["scale"])


def op_shard_demux(ml):
    return lambda e, t: _demux_out(e.demux(_shard(t), t["a_s"], t["a_e"], ok=t["ok"], max_len=ml, want_fpt=True))


def op_shard_demux_refine(ml, hr):
    def op(e, t):
        r, dwell, stats, idx = e.demux_refine(_shard(t), t["a_s"], t["a_e"], hr, ok=t["ok"], max_len=ml)
        return (*_demux_out(r), dwell, stats, idx)
    return op


def op_calibrate(e, t):
    n = int(t["row_len"].shape[0])
    out = torch.empty((n, STRIDE), dtype=torch.float32, device=e.tdev)
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    _lib.check(e.L.wdx_calibrate_adc_dev(e.ctx.handle, p(t["adc"]), None, p(t["row_len"]), STRIDE, n, p(t["offset"]),
                                         p(t["scale"]), p(out), e._stream()))
    return (out,)


# ---- the child's frame ------------------------------------------------------------------------------------------------------------

class Frame:
    """What every child does: the serial references on a second context (closed before the engine under test exists), the
    engine under test, the overtaking control, the calibrated delay."""

    def __init__(self, make_engine):
        self.make_engine = make_engine
        self.ref = make_engine()
        self.eng = None
        self.out = dict(ok=False, checked=[])

    def serial(self, op, inp, which="real"):
        assert self.eng is None, "the references are computed before the engine under test is created"
        return _serial(self.ref, op, inp, which)

    def start(self):
        """the engine under test and the control: from here on there is one context in the process"""
        self.ref.close()
        self.ref = None
        self.eng = self.make_engine()
        torch.cuda.synchronize()
        self.A, self.B, log = so.side_streams()
        cal = {k: v for k, v in so.calibrate().items() if k != "tensor"}
        self.out.update(control=log, delay_calibration=cal)
        print("overtaking control:", "; ".join(log))
        print("delay calibration:", cal)
        return self.eng

    def warm(self, stream, calls):
        """calls = [(op, inputs)]: once to grow every buffer (on the DECOY, so that what stale memory holds is not the answer),
        once more for the warm serial wall time -> the delay in ms"""
        with torch.cuda.stream(stream):
            for op, inp in calls:
                inp.fill("decoy")
                outs = op(self.eng, inp.t)
                stream.synchronize()
                del outs
            t0 = time.perf_counter()
            for op, inp in calls:
                outs = op(self.eng, inp.t)
                stream.synchronize()
                del outs
            wall = time.perf_counter() - t0
        return wall, so.delay_ms_for(wall)

    def done(self):
        self.out["ok"] = True
        print(json.dumps(self.out))
        self.eng.close()
        return 0


def _differs(a, b):
    return not _same(a, b)


# ---- (A) --------------------------------------------------------------------------------------------------------------------------

def child_A(group, n):
    n = int(n)
    large = n > 4096
    rd = _reads(n, 1, long_at=() if group == "adc" else (17, n - 2))
    ml = _max_len(rd)
    rows_in = None if group == "adc" else _row_inputs(rd)
    f = Frame(lambda: _engine(large=large))
    hr, hr_opt, hr_q2 = _hr(), _hr(optimal=True), _hr(1.1)
    # the optimal change-points kernel needs about 15 us a read: 8 200 reads would make the delay (20 x the serial time) 2.4 s.
    # With LARGE its variants run on 800 reads in launch slices of 300 (two whole slices and a partial one).
    opt_rd, opt_in = rd, rows_in
    if large and group in ("fingerprint", "demux"):
        opt_rd = _reads(OPTIMAL_LARGE, 1, long_at=(17, OPTIMAL_LARGE - 2))
        opt_in = _row_inputs(opt_rd)
    opt_ml = _max_len(opt_rd)

    def sliced(op):
        def run(e, t):
            e.ctx.set_option(_lib.OPT_MAX_LAUNCH_SLICE, 300)
            try:
                return op(e, t)
            finally:
                e.ctx.set_option(_lib.OPT_MAX_LAUNCH_SLICE, LAUNCH_SLICE)
        return run if large else op
    rule = _rule(f.ref)
    cases = []   # (name, op, inputs, exempt from the asynchrony check)
    if group == "fingerprint":
        sh = _shard_arrays(_reads(n, 1))
        adc_in = Inputs({k: sh[k] for k in ("adc", "row_len", "offset", "scale")})
        cases = [("fingerprint", op_fingerprint(ml), rows_in, False),
                 ("fingerprint_refine", op_fingerprint_refine(ml, hr), rows_in, False),
                 ("fingerprint_refine, unchanged consensus", op_fingerprint_refine(ml, hr), rows_in, False),
                 ("fingerprint_refine, changed consensus", op_fingerprint_refine(ml, hr_q2), rows_in, True),
                 ("fingerprint_refine, optimal_cpts", sliced(op_fingerprint_refine(opt_ml, hr_opt)), opt_in, False),
                 ("wdx_calibrate_adc_dev", op_calibrate, adc_in, False)]
    elif group == "demux":
        X = Inputs(dict(X=dtw_cases.nonfinite_reads(np.random.default_rng(3), n, K)))
        cases = [("demux", op_demux(ml), rows_in, False),
                 ("demux_refine", op_demux_refine(ml, hr), rows_in, False),
                 ("demux_refine, optimal_cpts", sliced(op_demux_refine(opt_ml, hr_opt)), opt_in, False),
                 ("dtw", op_dtw, X, False)]
    elif group == "nearest":
        st = (np.arange(n) % 11 == 3).astype(np.int32) * 3
        X = Inputs(dict(X=dtw_cases.nonfinite_reads(np.random.default_rng(4), n, K), st=st))
        cases = [("nearest", op_nearest(False, rule), X, False),
                 ("nearest, want_dist", op_nearest(True, rule), X, False),
                 ("demux_nearest", op_demux_nearest(ml, rule), rows_in, False)]
    elif group == "tails":
        Xn = np.random.default_rng(6).normal(size=(n, K))
        D = f.serial(op_dtw, Inputs(dict(X=dtw_cases.nonfinite_reads(np.random.default_rng(5), n, K))))[0]
        st = (np.arange(n) % 7 == 2).astype(np.int32) * 3
        dist_in, fpt_in = Inputs(dict(D=D)), Inputs(dict(X=Xn, st=st))
        cases = [("svm_predict", lambda e, t: e.svm_predict(t["D"]), dist_in, False),
                 ("mlp_predict", lambda e, t: e.mlp_predict(t["D"]), dist_in, False),
                 ("boost_predict", lambda e, t: e.boost_predict(t["X"], status=t["st"], want_raw=True), fpt_in, False),
                 ("demux_svm", op_demux_tail("svm", ml), rows_in, False),
                 ("demux_svm, no dist", op_demux_tail("svm", ml, want_dist=False), rows_in, False),
                 ("demux_mlp", op_demux_tail("mlp", ml), rows_in, False),
                 ("demux_boost", op_demux_tail("boost", ml), rows_in, False),
                 ("demux_boost, refine", op_demux_tail("boost_refine", ml), rows_in, False)]
    elif group == "adc":
        shard_in = Inputs(_shard_arrays(rd))
        cases = [("demux, AdcShard", op_shard_demux(ml), shard_in, False),
                 ("demux_refine, AdcShard", op_shard_demux_refine(ml, hr), shard_in, False),
                 ("demux_svm, AdcShard", op_demux_tail("svm", ml, shard=True), shard_in, False)]
    else:
        raise SystemExit("unknown group " + group)

    # the references (the changed-consensus call leaves 1.1 Q resident: the references are independent of what is resident)
    want = [f.serial(op, inp) for _, op, inp, _ in cases]
    for (name, op, inp, _), w in zip(cases, want):
        assert _differs(w, f.serial(op, inp, "decoy")), name + ": the decoy gives the real batch's results"
    if group in ("fingerprint", "demux") and not large:     # (the LARGE batch starts with the same reads)
        _against_the_oracle(group, rd, want[0])
    if group == "fingerprint":      # the plain branch fails reads with 1, 4 and 5, the refinement branch with 3 and 6 too
        seen = set(want[0][3].tolist()) | set(want[1][4].tolist())
        assert {0, 1, 3, 5, 6} <= seen, seen

    eng = f.start()
    for (name, op, inp, exempt), w in zip(cases, want):
        if name.endswith("consensus"):
            wall, ms = 0.0, last_ms      # (no warm-up in between: the consensus of the call before is the resident one)
        else:
            wall, ms = f.warm(f.A, [(op, inp)])
        last_ms = ms
        with torch.cuda.stream(f.A):
            ev = inp.late(f.A, ms)
            outs = op(eng, inp.t)
            pending = not ev.query()
            got = _read_back(outs)
        rec = dict(name=name, same=_same(got, w), pending=pending, exempt=exempt, serial_ms=round(wall * 1e3, 3), delay_ms=ms)
        print(rec)
        f.out["checked"].append(rec)
    return f.done()


def _against_the_oracle(group, rd, want):
    """the plain fingerprint / fingerprint + DTW references against the CPU oracle: the file does not rest on the device alone"""
    n = len(rd["idx"])
    beyond = (_windows(rd) > 16384) & (rd["ok"] != 0)       # the oracle knows no limit: those reads are status 5 on the device
    assert np.array_equal(beyond, rd["is_long"])            # ... and are not shown to it (ok = 0; their rows are not used)
    fpt, dwell, stats, status = orc.fingerprint_batch(rd["base"][rd["idx"]], rd["a_s"], rd["a_e"],
                                                      orc.SegParams(barcode_num_events=K, **ri.SEG), rd["ok"] * ~beyond)
    if group == "fingerprint":
        d_fpt, d_dwell, d_stats, d_status = want
    else:
        d_dist, d_call, d_status, _, d_fpt = want
    assert beyond.sum() >= 1 and (d_status[beyond] == 5).all(), d_status[beyond]
    assert np.array_equal(d_status[~beyond], status[~beyond])
    assert {0, 1, 4, 5} <= set(d_status.tolist()), np.bincount(d_status)
    ok = (status == 0) & ~beyond
    assert ok.sum() * 2 > n
    assert np.array_equal(_bits(d_fpt[ok]), _bits(fpt[ok]))
    if group == "fingerprint":
        assert np.array_equal(d_dwell[ok], dwell[ok]) and np.array_equal(_bits(d_stats[ok]), _bits(stats[ok]))
    else:
        Dref = orc.dtw_matrix(fpt[ok], _refs(), WINDOW, PENALTY)
        assert np.array_equal(_bits(d_dist[ok]), _bits(Dref))
        assert np.array_equal(d_call[ok], orc.argmin_rows(Dref)) and (d_call[d_status != 0] == -1).all()


# ---- (B) --------------------------------------------------------------------------------------------------------------------------

def _big_windows(seed):
    """four whole-row windows of 11 201 .. 16 384 samples (fp_big: beyond the exact kernel's LDS capacity), padding 0"""
    rng = np.random.default_rng(seed)
    lens = [11201, 12800, 14999, 16384]
    rows = np.full((4, 16392), np.nan, dtype=np.float32)
    for i, ln in enumerate(lens):
        rows[i, :ln] = (np.repeat(rng.normal(80, 15, ln // 40 + 1), 40)[:ln] + rng.normal(0, 2, ln)).astype(np.float32)
    return dict(rows=rows, a_s=np.zeros(4, np.int32), a_e=np.array(lens, np.int32), ok=np.ones(4, np.uint8))


def _long_windows(seed):
    """four windows of 20 000 samples (fp_long, WDX_OPT_LONG_WINDOWS)"""
    rng = np.random.default_rng(seed)
    rows = np.stack([li.step_row(rng, 20000) for _ in range(4)])
    return dict(rows=rows, a_s=np.full(4, li.PADDING, np.int32), a_e=np.full(4, 20000 - li.PADDING, np.int32), ok=np.ones(4, np.uint8))


def child_B(case):
    """steps = [(who, op, inputs)]: step 0 runs on the delayed stream behind late inputs, the others at once, `who` = "slow" /
    "fast" (the stream) or "host" (op(engine, None) is a host-buffer call on the context's own stream)"""
    make, timed = (lambda: _engine(with_models=False)), False
    if case in ("fp_ws", "engine_work"):
        r1, r2 = _reads(SMALL, 1), _reads(500 if case == "fp_ws" else 3000, 2)
        mk = op_fingerprint if case == "fp_ws" else op_demux
        steps = [("slow", mk(_max_len(r1)), _row_inputs(r1)), ("fast", mk(_max_len(r2)), _row_inputs(r2))]
    elif case in ("ref_buf", "ref_buf_optimal"):
        opt = case.endswith("optimal")
        n = 96 if opt else SMALL         # (the optimal kernel needs milliseconds for a read: three calls, 20 x their time as delay)
        r1, r2 = _reads(n, 1), _reads(n, 2)
        i1, i2 = _row_inputs(r1), _row_inputs(r2)
        steps = [("slow", op_fingerprint_refine(_max_len(r1), _hr(1.0, opt)), i1),
                 ("fast", op_fingerprint_refine(_max_len(r2), _hr(1.1, opt)), i2),
                 ("slow", op_fingerprint_refine(_max_len(r2), _hr(1.0, opt)), i2)]
    elif case in ("fp_big", "fp_long"):
        gen, stride = (_big_windows, 16392) if case == "fp_big" else (_long_windows, 20000)
        pr = (sig_proc.SegParams(barcode_num_events=K, padding=0) if case == "fp_big" else
              sig_proc.SegParams(barcode_num_events=K, padding=li.PADDING, **li.TRIPLES["rna002"]))
        make = lambda: _engine(np.random.default_rng(8).normal(size=(N_REFS, K)), with_models=False, params=pr,   # noqa: E731
                               long_windows=case == "fp_long")
        op = lambda e, t: e.fingerprint(t["rows"], t["a_s"], t["a_e"], ok=t["ok"], stride=stride, max_len=stride)   # noqa: E731
        steps = [("slow", op, Inputs(gen(21))), ("fast", op, Inputs(gen(22)))]   # (the decoy: the same four reads in another order)
    elif case == "adc_stage":
        r1, r2 = _reads(SMALL, 1), _reads(SMALL, 2)
        steps = [("slow", op_shard_demux(_max_len(r1)), Inputs(_shard_arrays(r1))),
                 ("fast", op_shard_demux(_max_len(r2)), Inputs(_shard_arrays(r2)))]
    elif case in ("dtw", "timed", "dtw_wavefront", "dtw_wide"):
        L, nref, n1, n2, kw, window = K, N_REFS, SMALL, 700, {}, WINDOW
        if case == "dtw_wavefront":
            nref, n1, n2 = 10, 16, 16
        if case == "dtw_wide":
            L, kw, window = 40, dict(wide_dtw=True), None
        refs = np.random.default_rng(8).normal(size=(nref, L))
        make = lambda: _engine(refs, with_models=False, window=window, params=sig_proc.SegParams(barcode_num_events=L), **kw)  # noqa: E731
        rng = np.random.default_rng(31)
        mkX = lambda n: dtw_cases.nonfinite_reads(rng, n, L) if n >= 200 else rng.normal(size=(n, L))   # noqa: E731
        steps = [("slow", op_dtw, Inputs(dict(X=mkX(n1)))), ("fast", op_dtw, Inputs(dict(X=mkX(n2))))]
        timed = case == "timed"
    elif case == "nearest_buf":
        refs = np.random.default_rng(8).normal(size=(40, 33))
        make = lambda: _engine(refs, with_models=False, params=sig_proc.SegParams(barcode_num_events=33))   # noqa: E731
        rng = np.random.default_rng(32)
        steps = [("slow", None, Inputs(dict(X=dtw_cases.nonfinite_reads(rng, 1000, 33)))),
                 ("fast", None, Inputs(dict(X=dtw_cases.nonfinite_reads(rng, 1000, 33))))]
    elif case == "svm_host_dtw":
        make = lambda: _engine()   # noqa: E731
        r1 = _reads(SMALL, 1)
        Xh, Yh = np.random.default_rng(33).normal(size=(500, K)), _refs()

        def host_dtw(e, _t):
            out, am = np.full((500, N_REFS), -1.0, dtype=np.float32), np.full(500, -1, dtype=np.int32)
            _lib.check(e.L.wdx_dtw_matrix(e.ctx.handle, _lib.ptr(Xh), 500, _lib.ptr(Yh), N_REFS, K, WINDOW, PENALTY, _lib.ptr(out),
                                          _lib.ptr(am)))
            return (out, am)
        steps = [("slow", op_demux_tail("svm", _max_len(r1), want_dist=False), _row_inputs(r1)), ("host", host_dtw, None)]
    else:
        raise SystemExit("unknown case " + case)

    f = Frame(make)
    if case == "nearest_buf":
        rule = _rule(f.ref)
        steps = [(who, op_nearest(False, rule), inp) for who, _, inp in steps]
    if timed:
        f.ref.kernel_timing(True)
        f.ref.kernel_time_reset()
    want = [_serial(f.ref, op, inp) if inp is not None else _read_back(op(f.ref, None)) for _, op, inp in steps]
    assert _differs(want[0], _serial(f.ref, steps[0][1], steps[0][2], "decoy")), "the decoy gives the real batch's results"
    if timed:
        torch.cuda.synchronize()
        f.ref.kernel_time_reset()
        for _, op, inp in steps:
            _serial(f.ref, op, inp)
        serial_ms, serial_launches = f.ref.kernel_time(_lib.K_DTW)
        assert serial_launches >= 2 and serial_ms > 0

    eng = f.start()
    for slow, fast, tag in ((f.A, f.B, "A delayed"), (f.B, f.A, "B delayed")):
        streams = dict(slow=slow, fast=fast)
        wall, ms = f.warm(slow, [(op, inp) for _, op, inp in steps if inp is not None])
        if case == "engine_work":
            eng._work = None            # the cached workspace tensor: regrown small by call 1, dropped and regrown by call 2
        if timed:
            eng.kernel_timing(True)
            eng.kernel_time_reset()
        for _, _, inp in steps[1:]:
            if inp is not None:
                inp.fill("real")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        outs = []
        with torch.cuda.stream(slow):
            ev = steps[0][2].late(slow, ms)
            flag.fill_(1)               # behind the delay, in front of call 1
            outs.append(steps[0][1](eng, steps[0][2].t))
        pending_after_first = not ev.query()
        for who, op, inp in steps[1:]:
            if who == "host":
                outs.append(op(eng, None))
                continue
            with torch.cuda.stream(streams[who]):
                outs.append(op(eng, inp.t))
        # work enqueued on the other stream BEHIND call 2 sees what the delayed stream wrote in front of call 1: the library
        # did wait for the earlier stream (by whatever means) before call 2 used the shared workspaces
        with torch.cuda.stream(fast):
            ordered = int(flag.cpu()[0]) == 1
        got = []
        for (who, _, _), o in zip(steps, outs):
            with torch.cuda.stream(streams.get(who, fast)):
                got.append(_read_back(o))
        rec = dict(case=case, roles=tag, same=all(_same(g, w) for g, w in zip(got, want)), ordered=ordered,
                   each=[_same(g, w) for g, w in zip(got, want)], call1_async=pending_after_first,
                   serial_ms=round(wall * 1e3, 3), delay_ms=ms)
        if timed:
            t_ms, launches = eng.kernel_time(_lib.K_DTW)
            rec.update(dtw_ms=t_ms, dtw_launches=launches, serial_launches=serial_launches)
            rec["same"] = rec["same"] and launches == serial_launches and t_ms > 0
            eng.kernel_timing(False)
        print(rec)
        f.out["checked"].append(rec)
    return f.done()


# ---- (C) --------------------------------------------------------------------------------------------------------------------------

def child_C(case):
    refs1 = _refs(1)
    refs2 = np.ascontiguousarray(refs1[::-1] * 1.05 + 0.02)
    r1, r2 = _reads(SMALL, 1), _reads(SMALL, 2)
    i1, i2 = _row_inputs(r1), _row_inputs(r2)
    ml1, ml2 = _max_len(r1), _max_len(r2)
    if case == "refs":
        ops = (op_demux(ml1), op_demux(ml2))
        replace = lambda e: e.set_refs(refs2, WINDOW, PENALTY)   # noqa: E731
        restore = lambda e: e.set_refs(refs1, WINDOW, PENALTY)   # noqa: E731
    else:
        kind = "boost" if case == "boost" else case
        ops = (op_demux_tail(kind, ml1), op_demux_tail(kind, ml2))
        new = {"svm": lambda: _svm(refs1, 6), "mlp": lambda: _mlp(refs1, 10), "boost": lambda: _boost(82)}[case]
        old = {"svm": lambda: _svm(refs1, 5), "mlp": lambda: _mlp(refs1, 9), "boost": lambda: _boost(81)}[case]
        replace = lambda e: getattr(e, "set_" + case)(new())   # noqa: E731
        restore = lambda e: getattr(e, "set_" + case)(old())   # noqa: E731
    f = Frame(lambda: _engine(refs1))
    want1 = f.serial(ops[0], i1)
    replace(f.ref)
    want2 = f.serial(ops[1], i2)
    assert _differs(want1, f.serial(ops[0], i1)), "the replacement changes nothing in call 1's outputs"
    restore(f.ref)
    assert _differs(want2, f.serial(ops[1], i2)), "the replacement changes nothing in call 2's outputs"
    assert _differs(want1, f.serial(ops[0], i1, "decoy"))

    eng = f.start()
    for slow, fast, tag in ((f.A, f.B, "A delayed"), (f.B, f.A, "B delayed")):
        restore(eng)
        wall, ms = f.warm(slow, [(ops[0], i1), (ops[1], i2)])
        i2.fill("real")
        with torch.cuda.stream(slow):
            i1.late(slow, ms)
            o1 = ops[0](eng, i1.t)
        replace(eng)                     # at once: call 1 is still behind its delay
        with torch.cuda.stream(fast):
            o2 = ops[1](eng, i2.t)
        with torch.cuda.stream(slow):
            g1 = _read_back(o1)
        with torch.cuda.stream(fast):
            g2 = _read_back(o2)
        rec = dict(case=case, roles=tag, same=_same(g1, want1) and _same(g2, want2), call1=_same(g1, want1), call2=_same(g2, want2),
                   serial_ms=round(wall * 1e3, 3), delay_ms=ms)
        print(rec)
        f.out["checked"].append(rec)
    return f.done()


# ---- (D) --------------------------------------------------------------------------------------------------------------------------

def child_D():
    rd = _reads(SMALL, 1)
    inp = _row_inputs(rd)
    op = op_demux(_max_len(rd))
    f = Frame(lambda: _engine(with_models=False))
    want = f.serial(op, inp)
    assert _differs(want, f.serial(op, inp, "decoy"))
    eng = f.start()
    wall, ms = f.warm(f.A, [(op, inp)])
    with torch.cuda.stream(f.A):
        ev = inp.late(f.A, ms)
        outs = op(eng, inp.t)
    pending = not ev.query()
    eng.ctx.synchronize(C.c_void_p(f.A.cuda_stream))
    with torch.cuda.stream(f.B):         # a copy on ANOTHER non-blocking stream waits for nothing: it sees what is there
        got = [_np(None if o is None else o.clone()) for o in outs]
    f.out.update(same=_same(got, want), pending_before_synchronize=pending, delay_ms=ms)
    assert f.out["same"] and pending, f.out
    return f.done()


# ---- (E) --------------------------------------------------------------------------------------------------------------------------

E_ROWS, E_STRIDE = 2048, 8192


def _e_minibatch(seed):
    """a page-locked minibatch of 2 048 x 8 192 float32 samples whose windows are the whole rows (the copy is the 2-D one: 64 MB):
    64 step signals, drawn 2 048 times"""
    from warpdemux_amd.pipeline import pinned_empty

    rng = np.random.default_rng(seed)
    base = np.stack([li.step_row(rng, E_STRIDE) for _ in range(64)])
    idx = np.concatenate([np.arange(64), rng.integers(0, 64, E_ROWS - 64)])
    mb = pinned_empty((E_ROWS, E_STRIDE), np.float32)
    mb[:] = base[idx]
    a_s = np.full(E_ROWS, li.PADDING, dtype=np.int32)
    a_e = np.full(E_ROWS, E_STRIDE - li.PADDING, dtype=np.int32)
    ok = np.ones(E_ROWS, dtype=np.uint8)
    ok[5::23] = 0
    return mb, a_s, a_e, ok, base


def child_E(case):
    from warpdemux_amd import _marshal

    L = _lib.load()
    p = sig_proc.SegParams(barcode_num_events=K, padding=li.PADDING, **li.TRIPLES["rna004"])
    pc = p.to_c()
    mb1, a_s, a_e, ok, base = _e_minibatch(41)
    mb2 = _e_minibatch(42)[0]
    fpt, _, _, status = orc.fingerprint_batch(base, a_s[:64], a_e[:64], orc.SegParams(barcode_num_events=K, padding=li.PADDING,
                                                                                      **li.TRIPLES["rna004"]))
    assert (status == 0).sum() >= 32, np.bincount(status)
    refs1 = np.ascontiguousarray(fpt[status == 0][:N_REFS]) + 0.01
    refs2 = np.ascontiguousarray(fpt[status == 0][N_REFS:2 * N_REFS]) + 0.01
    state1 = dict(refs=refs1, svm=_svm(refs1, 5), boost=_boost(81))
    new = dict(refs=refs2, svm=_svm(refs1, 6), boost=_boost(82))[case]
    want_bits = (_lib.WANT_BOOST | _lib.WANT_FPT) if case == "boost" else (_lib.WANT_SVM | _lib.WANT_DIST)
    k = 4 if case == "boost" else 3

    def put(ctx, what, v):
        if what == "refs":
            _marshal.set_refs(ctx, v, WINDOW, PENALTY)
        else:
            _marshal.set_model(ctx, v)

    def submit(ctx, mb):
        desc = _lib.MinibatchInC(_lib.addr(mb), E_ROWS, E_STRIDE, None, None, _lib.addr(a_s), _lib.addr(a_e), _lib.addr(ok))
        _lib.check(L.wdx_demux_submit_ex(ctx.handle, 0, C.byref(desc), C.byref(pc), N_REFS, want_bits))

    def wait(ctx):
        o = _marshal.outputs(E_ROWS, K, N_REFS, k, want_bits)
        out = _marshal.out_c(o)
        _lib.check(L.wdx_demux_wait_ex(ctx.handle, 0, C.byref(out)))
        return [o[name] for name in ("status", "call", "dist", "fpt", "prob", "pred", "conf")]

    def context():
        ctx = _lib.Context(0)
        for what in ("refs", "svm", "boost"):
            put(ctx, what, state1[what])
        return ctx

    # the references: serially, on a second context
    ref = context()
    submit(ref, mb1)
    first_want = wait(ref)
    put(ref, case, new)
    submit(ref, mb2)
    second_want = wait(ref)
    submit(ref, mb1)
    first_in_new_state = wait(ref)
    ref.close()
    states_differ = _differs(first_want, first_in_new_state)
    st = first_want[0]
    assert (st == 0).sum() * 2 > E_ROWS and (st[5::23] == 1).all(), np.bincount(st)

    ctx = context()
    submit(ctx, mb2)                                   # warm: the slot's buffers are grown
    wait(ctx)
    times = []                                         # the setter's own host time, nothing in flight: to the new state and back
    for _ in range(5):
        for v in (new, state1[case]):
            t0 = time.perf_counter()
            put(ctx, case, v)
            times.append(time.perf_counter() - t0)
    setter_s = float(np.median(times))
    t0 = time.perf_counter()
    submit(ctx, mb1)
    t3 = time.perf_counter()
    put(ctx, case, new)                                # at once: the batch is in flight
    first = wait(ctx)
    flight_s = time.perf_counter() - t3
    submit(ctx, mb2)
    second = wait(ctx)
    ctx.close()
    res = dict(ok=True, case=case, first_same=_same(first, first_want), second_same=_same(second, second_want),
               states_differ=states_differ, first_is_new_state=_same(first, first_in_new_state), setter_s=setter_s, flight_s=flight_s,
               setter_times_s=[round(x, 7) for x in times], submit_s=t3 - t0)
    print(json.dumps(res))
    return 0


def main(argv):
    _imports()
    return {"A": child_A, "B": child_B, "C": child_C, "D": child_D, "E": child_E}[argv[0]](*argv[1:])


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
