"""Where the device-resident entries write: every `wdx_*_dev` that computes for a caller, called through ctypes with every
array in a frame of tests/helpers/framed.py -- [guard | exactly the documented bytes | guard] -- and `d_work` exactly what the
matching `*_workspace_bytes` returns.

Per case: every guard of every argument is intact; every input is unchanged byte for byte; every output equals, bit for bit,
what the matching `DemuxEngine` method returns for the same reads on a second context with ordinary roomy tensors (those
methods are pinned to the oracle by the rest of the suite; the smallest plain fingerprint / demux case is compared with
oracle.wdx_oracle here as well).  Outputs start as 0xA5 bytes -- no legal status, call or index, and not the library's NaN --
so an element the call should have written and did not is a mismatch; the INCREMENTED histograms start at known non-zero
values.  Behind every float input lies NaN, behind every int16 input 32767.

The fused entries run with their d_work in four prior states -- 0x00, 0xFF, seeded random bytes, the leftover of a call with
another n -- and must give the same bits from each: DESIGN.md 7 lists, piece by piece, where a call writes d_work before it
reads it.  After a call the eight counters at the front of the fingerprint piece are read back from the payload (it is the
test's own memory); `test_the_lists_were_used` asserts that the slow, big0 and back lists each held reads in some case.

Shapes: the batch sizes on both sides of ld = round_up(n, 64), of the chain's threshold and of kRowMajorMinReads (8 192,
where the read-minor copy leaves the layout); K = 25 and an odd K; optional outputs given and NULL; launch slices; small
classifier blocks; shards of three slices whose last is shorter and on the other side of 8 192."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_nearest as tn
import test_gpu_streams as gs
from helpers import framed as fr
from helpers import refine_inputs as ri
from helpers.dtw_cases import RL, RM, TM, last_route
from warpdemux_amd import _lib, sig_proc

pytestmark = pytest.mark.gpu

K, N_REFS, STRIDE = gs.K, gs.N_REFS, gs.STRIDE
I_LONG, I_TAIL_LONG = 3, 17      # a window of 7 000 samples (beyond 6 144) | a barcode tail beyond kTailCap = 2 048 samples
CHAIN, SLICE = "chain", "slice"
STATES = ("zero", "ff", "random", "leftover")
COUNTERS = {}                    # case id -> the eight counters its call left


# ---- engines: `mine` lends its context to the ctypes calls, `ref` answers through its methods ---------------------------------------

@functools.lru_cache(maxsize=None)
def _engines(K_=K):
    gs._imports()
    if K_ == K:
        return gs._engine(), gs._engine()
    refs = np.ascontiguousarray(np.random.default_rng(K_).normal(size=(N_REFS, K_)))
    params = sig_proc.SegParams(barcode_num_events=K_, **ri.SEG)
    return tuple(gs._engine(refs, with_models=False, params=params) for _ in range(2))


def _set_options(engines, opts):
    for e in engines:
        for o, v in opts:
            e.ctx.set_option(o, v)


# ---- reads ----------------------------------------------------------------------------------------------------------------------

def _long_tail_row(seed):
    """a read of tests/helpers/refine_inputs.py's recipe whose 30 levels behind the consensus dwell 75 .. 100 samples each: the
    oracle matches the consensus (status 0) and puts sig_barcode_start ~2 600 samples before the window's end"""
    q, rng = ri.consensus(), np.random.default_rng(seed)
    lv = np.concatenate([rng.normal(0, 1, 4), q, rng.normal(0, 1, 30)]) * 12.0 + 85.0
    dw = np.concatenate([rng.integers(12, 40, 4 + q.size), rng.integers(75, 100, 30)])
    x = (np.repeat(lv, dw) + rng.normal(0, 1.5, int(dw.sum()))).astype(np.float32)
    assert x.size <= STRIDE - 200, x.size
    return x


@functools.lru_cache(maxsize=None)
def _reads(n, seed=1, special=True):
    """gs._reads with the reads that fill the pieces: a failed detection, a NaN inside a window, windows into the NaN tail
    (all of refine_inputs), windows beyond the main instantiation (its reads of more than 5 120 samples), one beyond 6 144
    samples and one barcode tail beyond kTailCap"""
    gs._imports()
    rd = gs._reads(n, seed, long_at=(I_LONG,) if special and n > I_LONG else ())
    if special:
        b = rd["b"]
        rd["base"][ri.I_NAN, :b["rows_nan"].shape[1]] = b["rows_nan"][ri.I_NAN]
        rd["long_row"][7000:] = np.nan
        rd["a_e"][rd["is_long"]] = 7000 - ri.PADDING
        x = _long_tail_row(seed)
        rd["base"][I_TAIL_LONG] = np.nan
        rd["base"][I_TAIL_LONG, :x.size] = x
        at = rd["idx"] == I_TAIL_LONG
        rd["a_s"][at], rd["a_e"][at], rd["ok"][at] = ri.PADDING, x.size - ri.PADDING, 1
    return rd


class Rows:
    """the framed inputs of one batch (float32 packed rows, or an int16 strided shard) and their device copies for the
    reference engine; `unchanged()` compares every frame's payload with what was put there"""

    def __init__(self, n, adc, seed=1):
        import torch

        rd = _reads(n, seed, special=not adc)
        self.n, self.adc, self.max_len = n, adc, gs._max_len(rd)
        host = gs._shard_arrays(rd) if adc else gs._packed(rd)
        self.frames = {k: fr.framed_input(v) for k, v in host.items()}
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}   # the reference's own copies
        if adc:
            f = self.frames
            self.desc = _lib.AdcDevInC(adc=f["adc"].ptr, row_off=None, stride=STRIDE, row_len=f["row_len"].ptr, offset=f["offset"].ptr,
                                       scale=f["scale"].ptr, row_win=None)
        torch.cuda.synchronize()

    def c_rows(self):
        if self.adc:
            return (C.byref(self.desc), self.max_len, self.n)
        return (self.frames["sig"].ptr, self.frames["off"].ptr, None, 0, self.max_len, self.n)

    def c_win(self):
        f = self.frames
        return (f["a_s"].ptr, f["a_e"].ptr, f["ok"].ptr)

    def sig(self):
        """what a DemuxEngine method takes as `sig`, and its keyword arguments"""
        t = self.dev
        if self.adc:
            return gs._shard(t), dict(ok=t["ok"], max_len=self.max_len)
        return t["sig"], dict(ok=t["ok"], offsets=t["off"], max_len=self.max_len)

    def unchanged(self):
        import torch

        return [k for k, f in self.frames.items() if not torch.equal(f.payload, self.dev[k].view(-1).view(torch.uint8))]

    def damage(self):
        return {k: f.damage() for k, f in self.frames.items() if f.damage()}


@functools.lru_cache(maxsize=6)
def _rows(n, adc=False, seed=1):
    return Rows(n, adc, seed)


# ---- the entries ------------------------------------------------------------------------------------------------------------------
# per entry: the outputs it writes (name -> dtype, shape by the case), the optional ones, the arguments between `p` and the stream,
# and what the matching DemuxEngine method answers, by the same names

def _shapes(c):
    return dict(fpt=("float64", (c.n, c.K)), dwell=("int64", (c.n, c.K)), stats=("float64", (c.n, 6)), status=("int32", (c.n,)),
                dist=("float32", (c.n, c.nY)), call=("int32", (c.n,)), idx=("int32", (c.n, 3)), best=("float32", (c.n, 2)),
                prob=("float64", (c.n, c.k)), pred=("int32", (c.n,)), conf=("float64", (c.n,)), raw=("float64", (c.n, c.dim)),
                counts=("int64", (c.bins,)), bad=("int64", (1,)))


INCREMENTED = ("counts", "bad")


class Call:
    """the frames of one call's outputs and rule inputs"""

    def __init__(self, n, K_, nY, k=1, dim=1, bins=None, omit=(), offset=False):
        self.n, self.K, self.nY, self.k, self.dim, self.bins, self.omit, self.offset = n, K_, nY, k, dim, bins or nY + 1, set(omit), offset
        self.out, self.extra = {}, {}

    def o(self, name):
        if name in self.omit:
            return None
        if name not in self.out:
            dtype, shape = _shapes(self)[name]
            f = fr.framed(shape, dtype, fr.OUT_FILL, offset=np.dtype(dtype).itemsize if self.offset else 0)
            if name in INCREMENTED:
                f.set(self.start(name))
            self.out[name] = f
        return self.out[name].ptr

    def start(self, name):
        dtype, shape = _shapes(self)[name]
        return (np.arange(int(np.prod(shape)), dtype=np.int64) * 3 + 7).reshape(shape)

    def inp(self, name, array):
        self.extra[name] = (fr.framed_input(array), np.ascontiguousarray(array).copy())
        return self.extra[name][0].ptr

    def damage(self):
        d = {k: f.damage() for k, f in self.out.items()}
        d.update({k: f.damage() for k, (f, _) in self.extra.items()})
        return {k: v for k, v in d.items() if v}

    def inputs_changed(self):
        return [k for k, (f, a) in self.extra.items() if not np.array_equal(f.numpy(a.dtype, a.shape).view(np.uint8), a.view(np.uint8))]


def _rule_host(nY):
    lab = (np.arange(nY, dtype=np.int32) // 2).astype(np.int32)
    G = (nY + 1) // 2
    return lab, G, np.linspace(0.0, 0.5, G, dtype=np.float32), np.linspace(60.0, 20.0, G, dtype=np.float32)


def _t(x):
    return None if x is None else x.cpu().numpy()


def _args_fingerprint(c, x):
    return (c.o("fpt"), c.o("dwell"), c.o("stats"), c.o("status"))


def _want_fingerprint(e, x, sig, kw, c):
    fpt, dwell, stats, status = e.fingerprint(sig, x.dev["a_s"], x.dev["a_e"], **kw)
    return dict(fpt=fpt, dwell=dwell, stats=stats, status=status)


def _args_fingerprint_refine(c, x):
    return (c.rp, c.o("fpt"), c.o("dwell"), c.o("stats"), c.o("idx"), c.o("status"))


def _want_fingerprint_refine(e, x, sig, kw, c):
    fpt, dwell, stats, idx, status = e.fingerprint_refine(sig, x.dev["a_s"], x.dev["a_e"], c.hr, **kw)
    return dict(fpt=fpt, dwell=dwell, stats=stats, idx=idx, status=status)


def _args_demux(c, x):
    return (c.o("fpt"), c.o("dwell"), c.o("stats"), c.o("status"), c.o("dist"), c.o("call"), c.o("counts"), c.work.ptr)


def _counts(c):
    import torch

    return torch.from_numpy(c.start("counts")).cuda()


def _want_demux(e, x, sig, kw, c):
    r = e.demux(sig, x.dev["a_s"], x.dev["a_e"], want_fpt=True, counts=_counts(c), **kw)
    want = _want_fingerprint(e, x, sig, kw, c)
    assert gs._same([_t(want["fpt"]), _t(want["status"])], [_t(r.fpt), _t(r.status)])
    want.update(dist=r.dist, call=r.call, counts=r.counts)
    return want


def _args_demux_refine(c, x):
    return (c.rp, c.o("fpt"), c.o("dwell"), c.o("stats"), c.o("idx"), c.o("status"), c.o("dist"), c.o("call"), c.o("counts"), c.work.ptr)


def _want_demux_refine(e, x, sig, kw, c):
    r, dwell, stats, idx = e.demux_refine(sig, x.dev["a_s"], x.dev["a_e"], c.hr, counts=_counts(c), **kw)
    return dict(fpt=r.fpt, dwell=dwell, stats=stats, idx=idx, status=r.status, dist=r.dist, call=r.call, counts=r.counts)


def _args_demux_nearest(c, x):
    lab, G, mm, md = _rule_host(c.nY)
    return (c.o("fpt"), c.o("dwell"), c.o("stats"), c.o("status"), c.inp("labels", lab), G, c.inp("min_margin", mm), c.inp("max_dist", md),
            c.o("dist"), c.o("call"), c.o("best"), c.o("counts"), c.work.ptr)


def _want_demux_nearest(e, x, sig, kw, c):
    r = e.demux_nearest(sig, x.dev["a_s"], x.dev["a_e"], want_dist=True, want_fpt=True, counts=_counts(c), **gs._rule(e), **kw)
    want = _want_fingerprint(e, x, sig, kw, c)
    want.update(dist=r.dist, call=r.call, best=r.best, counts=r.counts)
    return want


def _args_demux_svm(c, x):
    return (c.o("fpt"), c.o("status"), c.o("dist"), c.o("prob"), c.o("pred"), c.o("conf"), c.work.ptr, c.block_rows)


def _want_demux_svm(e, x, sig, kw, c):
    # (without d_dist the decision sums are taken in the DTW kernel's epilogue, in another order: tests/test_gpu_parity.py pins
    # the two forms to each other within 1e-12 -- so the reference is asked for the form the framed call takes)
    want_dist = "dist" not in c.omit
    prob, pred, conf, status, dist, fpt = e.demux_svm(sig, x.dev["a_s"], x.dev["a_e"], want_dist=want_dist, want_fpt=True, **kw)
    want = dict(prob=prob, pred=pred, conf=conf, status=status, fpt=fpt)
    if want_dist:
        want["dist"] = dist
    return want


def _args_demux_mlp(c, x):
    return (c.o("fpt"), c.o("status"), c.o("dist"), c.o("prob"), c.o("pred"), c.o("conf"), c.o("bad"), c.work.ptr, c.block_rows)


def _want_demux_mlp(e, x, sig, kw, c):
    import torch

    bad = torch.from_numpy(c.start("bad")).cuda()
    prob, pred, conf, status, dist, fpt = e.demux_mlp(sig, x.dev["a_s"], x.dev["a_e"], want_dist=True, want_fpt=True, n_nonfinite=bad, **kw)
    return dict(prob=prob, pred=pred, conf=conf, status=status, dist=dist, fpt=fpt, bad=bad)


def _args_demux_boost(c, x):
    return (c.rp, c.o("fpt"), c.o("idx") if c.rp else None, c.o("status"), c.o("raw"), c.o("prob"), c.o("pred"), c.o("conf"), c.work.ptr)


def _want_demux_boost(e, x, sig, kw, c):
    prob, pred, conf, status, idx, fpt, raw = e.demux_boost(sig, x.dev["a_s"], x.dev["a_e"], c.hr, want_fpt=True, want_raw=True, **kw)
    want = dict(prob=prob, pred=pred, conf=conf, status=status, fpt=fpt, raw=raw)
    if idx is not None:
        want["idx"] = idx
    return want


# name -> (C entry without wdx_ / _dev, arguments, reference, refines, needs d_work, outputs that may be NULL, classes from)
FUSED = {
    "fingerprint": ("fingerprint", _args_fingerprint, _want_fingerprint, False, False, ("fpt", "dwell", "stats"), None),
    "fingerprint_refine": ("fingerprint_refine", _args_fingerprint_refine, _want_fingerprint_refine, True, False, ("fpt", "dwell", "stats"), None),
    "demux": ("demux", _args_demux, _want_demux, False, True, ("fpt", "dwell", "stats"), None),
    "demux_refine": ("demux_refine", _args_demux_refine, _want_demux_refine, True, True, ("fpt", "dwell", "stats"), None),
    "demux_nearest": ("demux_nearest", _args_demux_nearest, _want_demux_nearest, False, True, ("fpt", "dwell", "stats", "dist"), None),
    "demux_svm": ("demux_svm", _args_demux_svm, _want_demux_svm, False, True, ("fpt", "dist"), "svm"),
    "demux_mlp": ("demux_mlp", _args_demux_mlp, _want_demux_mlp, False, True, ("fpt", "dist"), "mlp"),
    "demux_boost": ("demux_boost", _args_demux_boost, _want_demux_boost, False, True, ("fpt",), "boost"),
    "demux_boost_rp": ("demux_boost", _args_demux_boost, _want_demux_boost, True, True, ("fpt",), "boost"),
}
NO_ADC_TWIN = ("demux_nearest",)


def _work_bytes(mine, x, entry, refine, K_):
    L, h = mine.L, mine.ctx.handle
    if x.adc:
        f = L.wdx_demux_refine_adc_workspace_bytes if refine else L.wdx_demux_adc_workspace_bytes
        return int(f(h, x.n, x.max_len, K_))
    return int((L.wdx_demux_refine_workspace_bytes if refine else L.wdx_demux_workspace_bytes)(x.n, K_))


def _prior(mine, work, state, n, K_):
    """d_work's content before the call"""
    import torch

    if state == "zero":
        work.payload.zero_()
    elif state == "ff":
        work.payload.fill_(0xFF)
    else:
        g = torch.Generator(device="cuda")
        g.manual_seed(0xD1CE + n)
        work.payload.copy_(torch.randint(0, 256, (work.nbytes,), dtype=torch.uint8, device="cuda", generator=g))
        if state == "leftover":   # a plain demux call of other reads and another n, run in this very memory
            m = max(1, (n + 1) // 2)
            assert int(mine.L.wdx_demux_workspace_bytes(m, K_)) <= work.nbytes
            y = _rows(m, False, seed=2)
            roomy = Call(m, K_, mine.nY)
            roomy.work = work
            pc = mine.params.to_c()
            _lib.check(mine.L.wdx_demux_dev(mine.ctx.handle, *y.c_rows(), *y.c_win(), C.byref(pc), *_args_demux(roomy, y), None))
    torch.cuda.synchronize()


def _run_fused(name, n, *, adc=False, opts=(), omit=(), states=STATES, block_rows=0, offset=False, K_=K, case=None):
    import torch

    entry, args, want_of, refines, has_work, _optional, classes = FUSED[name]
    mine, ref = _engines(K_)
    x = _rows(n, adc)
    _set_options((mine, ref), opts)
    try:
        hr = gs._hr() if refines else None
        hr_c = hr.to_c() if refines else None
        sig, kw = x.sig()
        c0 = Call(n, K_, mine.nY, omit=omit)
        k, dim = {None: (1, 1), "svm": (mine.n_classes, 1), "mlp": (mine.mlp_classes, 1),
                  "boost": (mine.boost_classes, mine.boost_dim)}[classes] if K_ == K else (1, 1)
        c0.hr, c0.block_rows, c0.k, c0.dim = hr, block_rows, k, dim
        c0.bins = (mine.nY + 1) // 2 + 1 if name == "demux_nearest" else mine.nY + 1
        if name in ("demux_svm", "demux_mlp"):
            kw = dict(kw, block_rows=block_rows)
        want = {k_: _t(v) for k_, v in want_of(ref, x, sig, kw, c0).items()}
        torch.cuda.synchronize()
        fn = getattr(mine.L, "wdx_%s%s_dev" % (entry, "_adc" if adc else ""))
        # (wdx_demux_boost_dev without rp: "wdx_demux_workspace_bytes(n_reads, K) is enough")
        nbytes = _work_bytes(mine, x, entry, refines, K_) if has_work else 0
        first = None
        for state in (states if has_work else states[:1]):
            c = Call(n, K_, mine.nY, k, dim, c0.bins, omit, offset)
            c.hr, c.rp, c.block_rows = hr, (C.byref(hr_c) if refines else None), block_rows
            if has_work:
                c.work = fr.framed(nbytes, "uint8", 0, offset=16 if offset else 0)
                _prior(mine, c.work, state, n, K_)
            pc = mine.params.to_c()
            with mine.ctx.refine_options_for_call(hr):
                _lib.check(fn(mine.ctx.handle, *x.c_rows(), *x.c_win(), C.byref(pc), *args(c, x), None))
            torch.cuda.synchronize()
            what = (name, n, state)
            assert c.damage() == {} and x.damage() == {}, (what, c.damage(), x.damage())
            assert not has_work or c.work.damage() == [], (what, "d_work", c.work.damage())
            assert x.unchanged() == [] and c.inputs_changed() == [], (what, x.unchanged(), c.inputs_changed())
            got = {k_: f.numpy() for k_, f in c.out.items()}
            assert set(got) == set(want) - set(omit), (what, sorted(got), sorted(want))
            for k_, g in got.items():
                w = want[k_]
                assert g.dtype == w.dtype and g.shape == w.shape, (what, k_, g.dtype, g.shape, w.dtype, w.shape)
                same = gs._bits(g) == gs._bits(w)
                assert same.all(), (what, k_, "first mismatch at", np.argwhere(~same)[:4].tolist())
            if first is None:
                first = got
            assert gs._same(list(got.values()), list(first.values())), (what, "the result depends on what d_work held")
            if name in ("demux", "demux_refine") and not adc and case is not None:
                COUNTERS[case + "-" + state] = fr.counters(c.work, n, K_)
        return want
    finally:
        _set_options((mine, ref), [(o, 0) for o, _ in opts])


# ---- the cases --------------------------------------------------------------------------------------------------------------------

NS_ALL = (1, 63, 64, 65, 300, 2304, 8191, 8192, 8193)
NS_SOME = (65, 300, 2304, 8192)
OPTS = {None: (), CHAIN: ((_lib.OPT_FAST_CHAIN_MIN_READS, 1),), SLICE: ((_lib.OPT_MAX_LAUNCH_SLICE, 700),)}


def _fused_cases():
    out = []
    for name in FUSED:
        for n in (NS_ALL if name in ("demux", "demux_refine") else NS_SOME):
            out.append((name, n, None))
        out.append((name, 300, CHAIN))
        out.append((name, 2304, SLICE))
    return sorted(out, key=lambda c: c[1])   # (by batch size: the framed reads of one size serve every entry)


@pytest.mark.parametrize("name,n,how", _fused_cases(), ids=lambda v: str(v))
def test_fused_entry_stays_inside_its_buffers(name, n, how):
    _run_fused(name, n, opts=OPTS[how], case="%s-%d-%s" % (name, n, how))


@pytest.mark.parametrize("name", list(FUSED))
def test_optional_outputs_null_and_an_unaligned_base(name):
    """every optional output NULL (the fingerprints then live at the front of d_work), and every array at exactly the
    alignment include/wdx.h states: d_work 16 bytes off a 512-byte boundary, outputs one element off"""
    optional = FUSED[name][5]
    _run_fused(name, 65, omit=optional, states=("random", "leftover"))
    _run_fused(name, 300, omit=optional, opts=OPTS[CHAIN], states=("random",))
    _run_fused(name, 65, offset=True, states=("random",))


@pytest.mark.parametrize("name", ["demux_svm", "demux_mlp"])
def test_small_classifier_blocks(name):
    _run_fused(name, 300, block_rows=37, states=("random",))


@pytest.mark.parametrize("name", ["fingerprint", "demux"])
def test_an_odd_fingerprint_length(name):
    """K = 13: n K 8 is rarely a multiple of 256"""
    for n in (63, 65):
        _run_fused(name, n, K_=13, states=("random", "leftover"))


# shards: three slices, the last one shorter -- all below 8 192, and full slices from 8 192 on with the last below it (a last
# slice is never longer than a full one, so the other direction does not exist)
SHARDS = {"small": (800, 300), "across": (16484, 8192)}


@pytest.mark.parametrize("shape", list(SHARDS))
@pytest.mark.parametrize("name", [k for k in FUSED if k not in NO_ADC_TWIN])
def test_adc_twin_stays_inside_its_buffers(name, shape):
    n, slice_reads = SHARDS[shape]
    opts = ((_lib.OPT_ADC_DEV_SLICE_READS, slice_reads),)
    _run_fused(name, n, adc=True, opts=opts, states=("random", "ff") if shape == "small" else ("random",))
    assert (n - 1) // slice_reads + 1 == 3 and n % slice_reads != 0


def test_calibrate_adc_dev():
    import torch

    mine, ref = _engines()
    for n in (1, 65):
        x = _rows(n, True)
        want = _t(gs.op_calibrate(ref, x.dev)[0])
        out = fr.framed((n, STRIDE), "float32")
        f = x.frames
        _lib.check(mine.L.wdx_calibrate_adc_dev(mine.ctx.handle, f["adc"].ptr, None, f["row_len"].ptr, STRIDE, n, f["offset"].ptr,
                                                f["scale"].ptr, out.ptr, None))
        torch.cuda.synchronize()
        assert out.damage() == [] and x.damage() == {} and x.unchanged() == []
        assert np.array_equal(gs._bits(out.numpy()), gs._bits(want))
        a = gs._shard_arrays(_reads(n, 1, special=False))
        assert np.array_equal(gs._bits(out.numpy()), gs._bits(sig_proc.calibrate_adc(a["adc"], a["row_len"], a["offset"], a["scale"])))


# ---- tail-only entries ----------------------------------------------------------------------------------------------------------------

# route -> (nX, nY, L, window, wide, options, (family, layout, fused)): tests/test_gpu_nearest.py's ROUTES at the smallest nX of each
NO_WF = tn.NO_WF
ROUTES = {
    "short-rowmajor-fused": (131009, 6, 25, 15, False, (), ("short", RM, True)),
    "band8-fused": (131009, 6, 40, 8, False, (), ("band", RM, True)),
    "band32-fused": (131009, 6, 40, 32, False, (), ("band", RM, True)),
    "rowmajor-split": (8192, 6, 25, 15, False, (), ("short", RM, False)),
    "readminor-split": (2731, 6, 25, 15, False, (), ("short", TM, False)),
    "readminor-fused": (64, 1, 25, 15, False, NO_WF, ("short", TM, True)),
    "readminor-band15-fused": (65, 1, 40, 15, False, NO_WF, ("band", TM, True)),
    "gridy-split": (410, 40, 33, 15, False, (), ("band", TM, False)),
    "refs-as-lanes": (8, 200, 25, 15, False, NO_WF, ("short", RL, False)),
    "wavefront": (16, 10, 25, 15, False, (), ("wavefront", RM, False)),
    "scratch": (65, 5, 40, None, False, (), ("scratch", TM, False)),
    "wide-split": (65, 5, 40, None, True, (), ("wide", TM, False)),
    "wide-rowmajor-fused": (131009, 5, 40, None, True, (), ("wide", RM, True)),
    "wide-readminor-fused": (65, 1, 40, None, True, (), ("wide", TM, True)),
}
_MINE = {}


def _tail_engines(L, wide):
    from warpdemux_amd.engine import DemuxEngine

    key = (L, bool(wide))
    if key not in _MINE:
        _MINE[key] = DemuxEngine(np.zeros((1, L)), 15, 0.1, sig_proc.SegParams(barcode_num_events=L), wide_dtw=bool(wide))
    return _MINE[key], tn._engine(L, wide)


def _check(c, what, want):
    assert c.damage() == {} and c.inputs_changed() == [], (what, c.damage(), c.inputs_changed())
    for k_, w in want.items():
        g = c.out[k_].numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k_)
        same = gs._bits(g) == gs._bits(w)
        assert same.all(), (what, k_, np.argwhere(~same)[:4].tolist())


@pytest.mark.parametrize("route", list(ROUTES))
def test_dtw_matrix_and_nearest_dev_route_by_route(route):
    import torch

    nX, nY, L, window, wide, options, (family, layout, fused) = ROUTES[route]
    mine, ref = _tail_engines(L, wide)
    X, Y = tn._inputs(nX, nY, L, seed=sum(map(ord, route)))
    status = tn._status(nX, 7)
    labels, G = np.arange(nY, dtype=np.int32) % 3, 3
    mm, md = np.linspace(0.0, 0.5, G, dtype=np.float32), np.linspace(60.0, 20.0, G, dtype=np.float32)
    _set_options((mine, ref), options)
    try:
        for e in (mine, ref):
            e.set_refs(Y, window, 0.1)
        dX, st = torch.from_numpy(X).cuda(), torch.from_numpy(status).cuda()
        D, am = ref.dtw(dX)
        c = Call(nX, L, nY)
        _lib.check(mine.L.wdx_dtw_matrix_dev(mine.ctx.handle, c.inp("X", X), nX, c.o("dist"), c.o("call"), None))
        r = last_route(mine.ctx)
        assert (r.family, r.layout, r.fused) == (family, layout, fused), r
        torch.cuda.synchronize()
        _check(c, (route, "dtw_matrix_dev"), dict(dist=_t(D), call=_t(am)))
        for want_dist in (True, False):
            start = torch.from_numpy(np.arange(G + 1, dtype=np.int64) * 3 + 7).cuda()
            res = ref.nearest(dX, labels=labels, n_labels=G, min_margin=mm, max_dist=md, want_dist=want_dist, status=st, counts=start)
            c = Call(nX, L, nY, bins=G + 1, omit=() if want_dist else ("dist",))
            _lib.check(mine.L.wdx_nearest_dev(mine.ctx.handle, c.inp("X", X), nX, c.inp("status", status), c.inp("labels", labels), G,
                                              c.inp("min_margin", mm), c.inp("max_dist", md), c.o("dist"), c.o("call"), c.o("best"),
                                              c.o("counts"), None))
            r = last_route(mine.ctx)
            assert (r.family, r.layout, r.fused) == (family, layout, fused), r
            torch.cuda.synchronize()
            want = dict(call=_t(res.call), best=_t(res.best), counts=_t(res.counts))
            if want_dist:
                want["dist"] = _t(res.dist)
            _check(c, (route, "nearest_dev", want_dist), want)
    finally:
        _set_options((mine, ref), [(o, 0) for o, _ in options])


def _distances(n, nY, seed):
    """float32 rows as a DTW writes them, with an infinite and a NaN row when there is room"""
    D = np.abs(np.random.default_rng(seed).normal(20.0, 6.0, size=(n, nY))).astype(np.float32)
    if n > 3:
        D[2, 1], D[3, 0] = np.inf, np.nan
    return D


@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_svm_and_mlp_predict_dev(n):
    import torch

    mine, ref = _engines()
    D = _distances(n, mine.nY, n)
    dD = torch.from_numpy(D).cuda()
    prob, pred, conf = ref.svm_predict(dD)
    c = Call(n, K, mine.nY, k=mine.n_classes)
    _lib.check(mine.L.wdx_svm_predict_dev(mine.ctx.handle, c.inp("dist", D), n, c.o("prob"), c.o("pred"), c.o("conf"), None))
    torch.cuda.synchronize()
    _check(c, ("svm_predict_dev", n), dict(prob=_t(prob), pred=_t(pred), conf=_t(conf)))
    c = Call(n, K, mine.nY, k=mine.mlp_classes)
    bad = torch.from_numpy(c.start("bad")).cuda()
    prob, pred, conf = ref.mlp_predict(dD, n_nonfinite=bad)
    _lib.check(mine.L.wdx_mlp_predict_dev(mine.ctx.handle, c.inp("dist", D), n, c.o("prob"), c.o("pred"), c.o("conf"), c.o("bad"), None))
    torch.cuda.synchronize()
    _check(c, ("mlp_predict_dev", n), dict(prob=_t(prob), pred=_t(pred), conf=_t(conf), bad=_t(bad)))
    assert n <= 3 or int(bad[0]) > 7, "the non-finite rows were counted on top of the start value"


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_boost_predict_dev(n, kernel):
    import torch

    mine, ref = _engines()
    rng = np.random.default_rng(n)
    X = rng.normal(size=(n, K))
    status = (rng.integers(0, 5, n) == 0).astype(np.int32) * 3
    if n > 4:
        X[4, 7] = np.nan
    opts = ((_lib.OPT_BOOST_KERNEL, kernel),)
    _set_options((mine, ref), opts)
    try:
        prob, pred, conf, raw = ref.boost_predict(torch.from_numpy(X).cuda(), torch.from_numpy(status).cuda(), want_raw=True)
        c = Call(n, K, mine.nY, k=mine.boost_classes, dim=mine.boost_dim)
        _lib.check(mine.L.wdx_boost_predict_dev(mine.ctx.handle, c.inp("fpt", X), c.inp("status", status), n, c.o("raw"), c.o("prob"),
                                                c.o("pred"), c.o("conf"), None))
        torch.cuda.synchronize()
        _check(c, ("boost_predict_dev", n, kernel), dict(raw=_t(raw), prob=_t(prob), pred=_t(pred), conf=_t(conf)))
    finally:
        _set_options((mine, ref), [(o, 0) for o, _ in opts])


# ---- what the cases rest on ------------------------------------------------------------------------------------------------------------

def test_smallest_plain_case_against_the_oracle():
    """the reference engine's plain fingerprint + DTW at n = 65 -- what test_fused_entry_stays_inside_its_buffers compares the
    framed calls with -- against the CPU oracle: the file does not rest on the device alone"""
    gs._imports()
    from oracle import wdx_oracle as orc

    n = 65
    want = _run_fused("demux", n, states=("random",))
    rd = _reads(n)
    beyond = rd["is_long"]                      # 7 000 samples: the oracle gets that read's own row
    rows = np.full((n, gs.LONG), np.nan, dtype=np.float32)
    rows[:, :STRIDE] = rd["base"][rd["idx"]]
    rows[beyond] = rd["long_row"]
    fpt, dwell, stats, status = orc.fingerprint_batch(rows, rd["a_s"], rd["a_e"], orc.SegParams(barcode_num_events=K, **ri.SEG), rd["ok"])
    assert np.array_equal(want["status"], status), (want["status"], status)
    ok = status == 0
    assert ok.sum() * 2 > n and {0, 1} <= set(status.tolist())
    assert np.array_equal(gs._bits(want["fpt"][ok]), gs._bits(fpt[ok])) and np.array_equal(want["dwell"][ok], dwell[ok])
    assert np.array_equal(gs._bits(want["stats"][ok]), gs._bits(stats[ok]))
    Dref = orc.dtw_matrix(fpt[ok], gs._refs(), gs.WINDOW, gs.PENALTY)
    assert np.array_equal(gs._bits(want["dist"][ok]), gs._bits(Dref))
    assert np.array_equal(want["call"][ok], orc.argmin_rows(Dref)) and (want["call"][~ok] == -1).all()


def test_the_lists_were_used():
    """a test whose lists stayed empty proves nothing about them: slow, big0 and -- with refinement -- back held reads"""
    for name, n, how in (("demux", 300, CHAIN), ("demux", 2304, None), ("demux_refine", 300, CHAIN), ("demux_refine", 2304, None)):
        case = "%s-%d-%s" % (name, n, how)
        if case + "-random" not in COUNTERS:
            _run_fused(name, n, opts=OPTS[how], states=("random",), case=case)
    seen = {k: v for k, v in COUNTERS.items() if k.endswith("-random")}
    print(seen)
    plain = [v for k, v in seen.items() if k.startswith("demux-")]
    refine = [v for k, v in seen.items() if k.startswith("demux_refine-")]
    assert any(v["slow"] > 0 for v in plain), plain
    assert any(v["big0"] > 0 for v in plain + refine), plain + refine
    assert any(v["back"] > 0 for v in refine), refine
    assert all(max(v.values()) <= int(k.split("-")[1]) for k, v in seen.items()), "a counter beyond the batch size"


def test_the_table_names_every_device_entry():
    """every wdx_*_dev of the library that computes for a caller has a row here; a new entry without one fails
    (the wdx_*_device entries have the sibling table tests/helpers/device_entries.py)"""
    diagnostics = ("profile", "selftest_", "calib_read", "synth_")
    lib = {e for e in _lib.EXPORTS if e.endswith("_dev") and not any(d in e for d in diagnostics)}
    fused = {"wdx_%s_dev" % v[0] for v in FUSED.values()}
    twins = {"wdx_%s_adc_dev" % v[0] for k, v in FUSED.items() if k not in NO_ADC_TWIN}
    tails = {"wdx_calibrate_adc_dev", "wdx_dtw_matrix_dev", "wdx_nearest_dev", "wdx_svm_predict_dev", "wdx_mlp_predict_dev",
             "wdx_boost_predict_dev"}
    assert fused | twins | tails == lib, sorted((fused | twins | tails) ^ lib)
