"""Every `wdx_*_device` entry in exact buffers, and the stream contract where the entries' own files do not hold it yet.  The rows,
their arguments by role, their cases and the rules come from tests/helpers/device_entries.py; tests/test_device_entry_table_host.py
closes that table against `_lib.EXPORTS` and include/wdx.h.  The sibling of tests/test_gpu_buffer_bounds.py and tests/test_gpu_streams.py,
which are closed over the `_dev` names.

Exact buffers (`test_exact_buffers`), per case of every row: every device array in a frame of tests/helpers/framed.py -- [guard |
exactly the documented bytes | guard] --, inputs with NaN behind them and NaN in their pad columns, outputs 0xA5.  Asserted per call:
every guard intact; every input unchanged byte for byte; every output bit for bit what the `DemuxEngine` method returns on a second
context with roomy tensors (wdx_svm_cv_couple_device: what the same ctypes entry returns there -- its method, svm_cross_val, runs a
whole cross-validation in front of the call; likewise the NULL-histogram calls of the `thr_ws` stream case), and (but for wdx_mlp_fit_device, whose rule helper is float64, and wdx_svm_cv_couple_device, whose coupling
has no bit-for-bit restatement: the table says what holds it) the NumPy rule; every element the header calls "not written" still what
it held.  A matrix with a leading dimension ends on element (rows-1) ld + cols - 1.  Each case runs
  * on a FRESH context and on a LEFTOVER one that has just run the same entry at a larger, different shape (the grow-only workspaces
    of the context start from that call's remains);
  * with every frame on its 512-byte boundary and one element off it;
  * with its nullable outputs all given and all NULL -- for wdx_accuracy_thresholds_device the NULL form right behind a call with
    k = 16 and R = 500 on the context's own histograms.

The stream contract (every body in a `run_child` child, which first proves that its side streams overtake):
  * late inputs on one side stream for the four entries no other file holds to it: the result is the serial call's on a second
    context, and the two that do not block return with the delay still running (wdx_mlp_fit_device and wdx_boost_fit_device block by
    contract and are exempt, as the blocking cases of tests/test_gpu_streams.py are);
  * two streams on one context, one shared buffer per case: call 1 behind the delay on one stream, call 2 at once on the other, then
    with the streams and the calls swapped; both equal their serial results."""
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
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

from helpers import device_entries as de  # noqa: E402
from helpers import framed as fr  # noqa: E402
from helpers import stream_order as so  # noqa: E402

pytestmark = pytest.mark.gpu


def _imports():
    global torch, _lib, DemuxEngine
    import torch
    from warpdemux_amd import _lib
    from warpdemux_amd.engine import DemuxEngine


def _engine():
    _imports()
    return DemuxEngine(np.random.default_rng(0).normal(size=(4, de.L_DTW)), de.WINDOW, de.PENALTY)


@functools.lru_cache(maxsize=None)
def _shared():
    """(the context the leftover calls run on, the second context that answers through DemuxEngine's methods)"""
    return _engine(), _engine()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize]) if a.dtype.kind in "fiub" else a


def _same(got, want, dtype=None):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if dtype is not None and want.dtype.kind in "iu" and np.dtype(dtype).kind in "iu":
        want = want.astype(dtype)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _first_difference(got, want):
    if got.shape != want.shape or got.dtype.kind != want.dtype.kind:
        return "%s %s against %s %s" % (got.dtype, got.shape, want.dtype, want.shape)
    bad = np.flatnonzero(_bits(got) != _bits(want.astype(got.dtype)))
    return "%d of %d elements, the first at %d: %r against %r" % (bad.size, got.size, int(bad[0]), got[bad[0]], want[bad[0]]) if bad.size else "dtype"


def _raw(f):
    """the payload's bytes on the host"""
    return f.payload.cpu().numpy()


# ---- one call in exact frames ---------------------------------------------------------------------------------------------------------

def _call_framed(case, eng, shift, null):
    """the case through ctypes on `eng`, every device array in a frame (`shift`: one element off its 512-byte boundary; `null`: the
    nullable outputs NULL) -> (frames, host outputs)"""
    off = lambda name, a: case.offsets.get(name, 0) + (np.dtype(a).itemsize if shift else 0)   # noqa: E731
    frames = {}
    for name, a in {**case.inputs, **case.inouts}.items():
        frames[name] = fr.framed_input(a, offset=off(name, a.dtype))
    for name, (count, dtype) in case.outputs.items():
        if not (null and name in case.nullable):
            frames[name] = fr.framed((count,), dtype, offset=off(name, dtype))
    p = {name: None for name in list(case.null_in) + list(case.outputs)}
    p.update({name: f.ptr for name, f in frames.items()})
    torch.cuda.synchronize()
    host = case.call(eng.L, eng.ctx.handle, p, eng._stream())
    torch.cuda.synchronize()
    return frames, host


def _check(case, frames, host, ref, rule, what):
    for name, f in frames.items():
        assert f.damage() == [], "%s: %s: a guard was written: %s" % (what, name, f.damage())
    for name, a in case.inputs.items():
        assert np.array_equal(_raw(frames[name]), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), "%s: input %s was written" % (what, name)
    got = {}
    for name, f in frames.items():
        if name in case.inputs:
            continue
        dtype = case.outputs[name][1] if name in case.outputs else case.inouts[name].dtype
        got[name] = f.numpy(dtype).reshape(-1)
        mask = case.written.get(name)
        if mask is not None:
            before = np.full(f.nbytes, fr.OUT_FILL, np.uint8) if name in case.outputs else np.ascontiguousarray(case.inouts[name]).view(np.uint8)
            size = np.dtype(dtype).itemsize
            kept = _raw(f).reshape(-1, size)[~mask]
            assert np.array_equal(kept, before.reshape(-1, size)[~mask]), "%s: %s: an element the header calls not written was written" % (what, name)
    got.update({k: np.asarray(v) for k, v in host.items()})
    for source, want in (("the second context", ref), ("the rule", rule)):
        if want is None:
            continue
        for name, g in got.items():
            mask = case.written.get(name)
            w = np.asarray(want[name]).reshape(-1)
            g1, w1 = (g, w) if mask is None else (g[mask], w[mask])
            assert _same(g1, w1, g.dtype), "%s: %s differs from %s: %s" % (what, name, source, _first_difference(g1, w1))
    if case.check is not None:
        case.check(got)
    return got


_BIG = {}


def _leave_leftover(name, case, eng):
    """the same entry at a larger, different shape on `eng`, in frames as well: what its workspaces hold afterwards is the leftover"""
    key = (name, case.options)
    if key not in _BIG:
        _BIG[key] = case.big()
    big = _BIG[key]
    frames, _ = _call_framed(big, eng, 0, big.nullable and case.null_big)
    for arg, f in frames.items():
        assert f.damage() == [], "%s big: %s: a guard was written: %s" % (name, arg, f.damage())


@pytest.mark.parametrize("name,cid", de.case_ids(), ids=["%s-%s" % (n[4:-7], c) for n, c in de.case_ids()])
def test_exact_buffers(name, cid):
    case = de.case(name, cid)
    mine, ref_eng = _shared()
    engines = [mine, ref_eng]
    t0 = time.time()
    try:
        for e in engines:
            for o, v in case.options:
                e.ctx.set_option(o, v)
        ref = de.finish(case, case.engine(ref_eng, de.tensors(torch, case)))
        rule = case.rule() if case.rule is not None else None
        runs = [("fresh", 0, False), ("fresh", 1, bool(case.nullable))]
        if case.big is not None:
            runs += [("leftover", 0, bool(case.nullable)), ("leftover", 1, False)]
        for state, shift, null in runs:
            if state == "fresh":
                eng = _engine()
                engines.append(eng)
                for o, v in case.options:
                    eng.ctx.set_option(o, v)
            else:
                eng = mine
                _leave_leftover(name, case, eng)
            what = "%s %s [%s context, %s, %s]" % (name, cid, state, "one element off 512 bytes" if shift else "on 512 bytes",
                                                   "nullable outputs NULL" if null else "every output given")
            frames, host = _call_framed(case, eng, shift, null)
            _check(case, frames, host, ref, rule, what)
            if state == "fresh":
                eng.close()
                engines.remove(eng)
    finally:
        for e in engines[:2]:
            for o, _ in case.options:
                e.ctx.set_option(o, 0)
        for e in engines[2:]:
            e.close()
    print("%s %s: %.2f s" % (name, cid, time.time() - t0))


# ---- the stream contract --------------------------------------------------------------------------------------------------------------

LATE = de.LATE_HERE   # entry -> (case, blocks by contract); tests/test_device_entry_table_host.py: every row has such a case somewhere

TWO = ("dtw_scratch", "self_ws", "medoid_ws", "svm_tables", "thr_ws")


def _child(*args):
    res, _ = so.run_child(HERE, args, timeout=150.0)
    assert res.get("ok") is True, res
    return res


@pytest.mark.parametrize("name", sorted(LATE))
def test_late_inputs_on_one_side_stream(name):
    res = _child("late", name)
    assert res["same"] and res["decoy_differs"] and (res["pending"] or res["exempt"]), res
    assert res["exempt"] == LATE[name][1], res


@pytest.mark.parametrize("case", TWO)
def test_two_streams_share_one_context(case):
    res = _child("two", case)
    assert len(res["checked"]) == 2 and all(c["same"] and c["ordered"] for c in res["checked"]), res


# ==== from here on: the child process ============================================================================================

def _decoy(case):
    """another valid batch of the same sizes: every float array halved and shifted (NaN stays NaN), the integer arrays as they are"""
    return {name: (a * 0.5 + 0.1 if a.dtype.kind == "f" else a) for name, a in {**case.inputs, **case.inouts}.items()}


def _differs(a, b):
    return any(not _same(a[k], b[k]) for k in a)


class _Op:
    """one call of a two-stream case: the table's case, or a call that is no `_device` entry"""

    def __init__(self, case):
        self.case = case
        self.real, self.decoy = de.tensors(torch, case), de.tensors(torch, case, _decoy(case))
        self.names = [n for n in self.real if ":" not in n]

    def serial(self, ref, values):
        """the call on `ref`, on the default stream, with the real batch or the decoy"""
        return de.finish(self.case, self.case.engine(ref, de.tensors(torch, self.case, None if values == "real" else _decoy(self.case))))

    def late(self, stream, ms):
        self.t = de.tensors(torch, self.case)
        return so.late(stream, [self.t[n] for n in self.names], [self.real[n] for n in self.names], [self.decoy[n] for n in self.names], ms)

    def now(self):
        self.t = de.tensors(torch, self.case)

    def run(self, eng):
        return self.case.engine(eng, self.t)


def _dtw_case(n=300):
    """wdx_dtw_matrix_dev through DemuxEngine.dtw: the call that shares ctx->scratch with the medoids"""
    X = np.random.default_rng(17).normal(size=(n, de.L_DTW))

    def engine(eng, t):
        dist, am = eng.dtw(t["X"].view(n, de.L_DTW))
        return dict(dist=dist, argmin=am)

    return de.Case("dtw_matrix_dev", None, engine, inputs=dict(X=X.reshape(-1)))


def _two_ops(case):
    c = de.case
    if case == "dtw_scratch":
        return _Op(_dtw_case()), _Op(c("wdx_medoids_device", "status"))
    if case == "self_ws":
        return _Op(c("wdx_self_matrix_device", "n65-ld68")), _Op(c("wdx_self_nearest_device", "n130-labels-tiles"))
    if case == "medoid_ws":
        return _Op(c("wdx_medoids_device", "status")), _Op(c("wdx_dba_step_device", "window15-band"))
    if case == "svm_tables":
        return _Op(c("wdx_svm_solve_device", "m40-ld41")), _Op(c("wdx_svm_cv_couple_device", "rows7-k7-mid"))
    assert case == "thr_ws"
    ops = []
    for cid in de.THR_WS_PAIR:                                # the context's own histograms at one (k, R), then at another
        base = c("wdx_accuracy_thresholds_device", cid)

        def engine(eng, t, base=base):
            o = dict(d_thr=torch.zeros(base.outputs["d_thr"][0], dtype=torch.float64, device="cuda"))
            base.call(eng.L, eng.ctx.handle, dict(d_prob=t["d_prob"].data_ptr(), d_y_idx=t["d_y_idx"].data_ptr(), d_thr=o["d_thr"].data_ptr(),
                                                  d_kept=None, d_hit=None, d_skipped=None), eng._stream())
            return o

        ops.append(_Op(de.Case(cid, base.call, engine, inputs=base.inputs, outputs=dict(d_thr=base.outputs["d_thr"]))))
    return ops


def _warm(eng, ops):
    """every call once (buffers sized, kernels loaded), then timed -> the delay that covers them"""
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.time()
        for op in ops:
            op.now()
            op.run(eng)
        torch.cuda.synchronize()
        wall = time.time() - t0
    return so.delay_ms_for(wall)


def _child_late(name):
    _imports()
    cid, exempt = LATE[name]
    A, B, log = so.side_streams()
    print("\n".join(log))
    eng, ref = _engine(), _engine()
    op = _Op(de.case(name, cid))
    serial, wrong = op.serial(ref, "real"), op.serial(ref, "decoy")
    ms = _warm(eng, [op])
    ev = op.late(A, ms)
    with torch.cuda.stream(A):
        res = op.run(eng)
        pending = not ev.query()                     # the call came back with the delay still running
        got = de.finish(op.case, res)                # (copies on A: they wait for A alone)
    same = not _differs(got, serial)
    eng.close(), ref.close()
    print(json.dumps(dict(ok=True, entry=name, case=cid, same=same, pending=pending, exempt=exempt, decoy_differs=_differs(wrong, serial), delay_ms=ms)))


def _child_two(case):
    _imports()
    A, B, log = so.side_streams()
    print("\n".join(log))
    eng, ref = _engine(), _engine()
    ops = _two_ops(case)
    want = [op.serial(ref, "real") for op in ops]
    assert _differs(want[0], ops[0].serial(ref, "decoy")) and _differs(want[1], ops[1].serial(ref, "decoy")), "a decoy gives the real batch's results"
    checked = []
    for slow, fast, order, tag in ((A, B, (0, 1), "call 1 delayed on A"), (B, A, (1, 0), "call 2 delayed on B")):
        first, second = ops[order[0]], ops[order[1]]
        ms = _warm(eng, [first, second])
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        second.now()
        torch.cuda.synchronize()
        with torch.cuda.stream(slow):
            ev = first.late(slow, ms)
            flag.fill_(1)                            # behind the delay, in front of the delayed call
            r1 = first.run(eng)
        pending = not ev.query()
        with torch.cuda.stream(fast):
            r2 = second.run(eng)
            ordered = int(flag.cpu()[0]) == 1        # the library waited for the earlier stream before it shared a buffer
            g2 = de.finish(second.case, r2)
        with torch.cuda.stream(slow):
            g1 = de.finish(first.case, r1)
        same = [not _differs(g1, want[order[0]]), not _differs(g2, want[order[1]])]
        checked.append(dict(roles=tag, same=all(same), each=same, ordered=ordered, delayed_call_async=pending, delay_ms=ms))
        torch.cuda.synchronize()
    eng.close(), ref.close()
    print(json.dumps(dict(ok=True, case=case, checked=checked)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "late":
        _child_late(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "two":
        _child_two(sys.argv[2])
    else:
        raise SystemExit("usage: test_gpu_device_entries.py late <entry> | two <case>")
