"""int16 ADC shards that stay on the device (`engine.AdcShard`, the *_adc_dev entries of include/wdx.h): every `DemuxEngine`
method on a shard against the same method on the float32 rows the shard stands for (`sig_proc.calibrate_adc`) -- every
output bit for bit (`_same`: dtype, shape, np.array_equal with NaN == NaN).  The strided and the packed layout, several
slices with a partial last one (OPT_ADC_DEV_SLICE_READS) and the built-in slice, the long-window options, the refinement
branch, the three classifier tails, reuse of the staging block across calls, the empty shard.  Inputs:
tests/helpers/adc_inputs.py and refine_inputs.py, the models of tests/helpers/{svm,mlp,boost}_ref.py."""
import functools

import numpy as np
import pytest

from helpers import adc_inputs, boost_ref, mlp_ref, svm_ref
from helpers import refine_inputs as ri
from warpdemux_amd import _lib, models, sig_proc

pytestmark = pytest.mark.gpu
K = 25
LAYOUTS = ("strided", "packed")


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t) for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _all_same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), (what, i)


def _d(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _batch(name):
    if name == "main":
        b = adc_inputs.main_batch()
    elif name == "long":
        b = adc_inputs.long_batch()
    elif name == "long40k":
        # the long batch (its 16 385-sample read is fingerprinted with the long-window option) and one 40 000-sample window
        base = adc_inputs.long_batch()
        rng = np.random.default_rng(40)
        lens = base["row_len"].tolist() + [40000]
        n, stride = len(lens), 40008
        mb = np.full((n, stride), np.nan, dtype=np.float32)
        mb[:-1, :base["adc"].shape[1]] = sig_proc.calibrate_adc(base["adc"], base["row_len"], base["offset"], base["scale"])
        mb[-1, :40000] = (np.repeat(rng.normal(80, 15, 1001), 40)[:40000] + rng.normal(0, 2, 40000)).astype(np.float32)
        adc, row_len, offset, scale = adc_inputs.quantise(mb, 41)
        assert row_len.tolist() == lens
        b = dict(adc=adc, row_len=row_len, offset=offset, scale=scale, a_s=np.zeros(n, dtype=np.int32),
                 a_e=np.array(lens, dtype=np.int32), ok=None, padding=0)
    else:
        b = ri.batch(int(name[len("refine"):]))
    b = dict(b)
    b["rows"] = sig_proc.calibrate_adc(b["adc"], b["row_len"], b["offset"], b["scale"])
    return b


def _shard(b, layout):
    """(AdcShard on the device, a_start, a_end) of a batch in one of the two layouts; the packed one holds the windows only,
    as tests/helpers/adc_inputs.pack_rows cuts them, with row_win for the windows that run into the NaN tail"""
    from warpdemux_amd.engine import AdcShard

    if layout == "strided":
        return AdcShard(_d(b["adc"]), _d(b["row_len"]), _d(b["offset"]), _d(b["scale"])), _d(b["a_s"]), _d(b["a_e"])
    flat, row_off, r_len, r_win, a_s2, a_e2 = adc_inputs.pack_rows(b)
    assert (row_off % 8 == 0).all()
    flat = np.concatenate([flat, np.full(8, 999, dtype=np.int16)])      # (never an empty tensor; never read)
    return (AdcShard(_d(flat), _d(r_len), _d(b["offset"]), _d(b["scale"]), offsets=_d(row_off), row_win=_d(r_win)),
            _d(a_s2), _d(a_e2))


@functools.lru_cache(maxsize=None)
def _engine(kind):
    """one engine per parameter set: plain (padding 100 / 0), the long-window options on, the tRNA set"""
    from warpdemux_amd.engine import DemuxEngine

    refs = np.random.default_rng(8).normal(size=(10, K))
    if kind == "refine":
        return DemuxEngine(refs, 15, 0.1, sig_proc.SegParams(barcode_num_events=K, **ri.SEG))
    pad = {"pad100": 100, "pad0": 0, "long": 0}[kind]
    return DemuxEngine(refs, 15, 0.1, sig_proc.SegParams(barcode_num_events=K, padding=pad), long_windows=kind == "long")


class _slices:
    """OPT_ADC_DEV_SLICE_READS for the duration of a block (0 = the built-in slice)"""

    def __init__(self, eng, reads):
        self.eng, self.reads = eng, reads

    def __enter__(self):
        self.eng.ctx.set_option(_lib.OPT_ADC_DEV_SLICE_READS, self.reads)

    def __exit__(self, *exc):
        self.eng.ctx.set_option(_lib.OPT_ADC_DEV_SLICE_READS, 0)


def _demux_outputs(eng, sig, a_s, a_e, ok, **rows):
    """every output of the plain entries: wdx_demux[_adc]_dev's through `demux` (counts INCREMENTED from a non-zero start),
    dwell and stats through `fingerprint`"""
    import torch

    counts = torch.arange(eng.nY + 1, dtype=torch.int64, device=eng.tdev) * 7
    r = eng.demux(sig, a_s, a_e, ok=ok, counts=counts, want_fpt=True, **rows)
    fpt, dwell, stats, status = eng.fingerprint(sig, a_s, a_e, ok=ok, **rows)
    torch.cuda.synchronize()
    assert _same(fpt, r.fpt) and _same(status, r.status)
    return r.status, r.fpt, r.dist, r.call, r.counts, dwell, stats


@functools.lru_cache(maxsize=None)
def _float32_demux(kind, name):
    b = _batch(name)
    stride = b["rows"].shape[1]
    return _demux_outputs(_engine(kind), _d(b["rows"]), _d(b["a_s"]), _d(b["a_e"]), _d(b["ok"]), stride=stride, max_len=stride)


@pytest.mark.parametrize("slice_reads", [100, 0], ids=["slices-of-100", "built-in-slice"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name,kind", [("main", "pad100"), ("long", "pad0")])
def test_plain_demux_equals_the_float32_twin(name, kind, layout, slice_reads):
    """256 reads with failed and garbage detections, inverted windows, NaN-tail windows and every start residue mod 8 (three
    slices of 100, the last partial); windows at 5 120 / 6 144 / 8 192 / 16 384 / 16 385"""
    eng, b = _engine(kind), _batch(name)
    want = _float32_demux(kind, name)
    shard, a_s, a_e = _shard(b, layout)
    max_len = b["rows"].shape[1]
    with _slices(eng, slice_reads):
        got = _demux_outputs(eng, shard, a_s, a_e, _d(b["ok"]), max_len=max_len)
        n_slices = -(-len(b["a_s"]) // slice_reads) if slice_reads else 1
        # rows of round_up(min(max_len, the 16 384-sample limit) + 8, 8) floats and three int32 per read of the largest slice
        pitch = (min(max_len, sig_proc.MAX_ADAPTER_SAMPLES) + 8 + 7) // 8 * 8
        assert eng.adc_staging_bytes(len(b["a_s"]), max_len) == min(len(b["a_s"]), slice_reads or 1 << 40) * (pitch * 4 + 12)
    _all_same(got, want, (name, layout, slice_reads))
    status = want[0].cpu().numpy()
    if name == "main":
        assert n_slices == (3 if slice_reads else 1)
        assert (status[5::23] == 1).all() and status[28] == 1 and (status == 0).sum() * 2 >= len(status)
        assert status[11] != 0 and status[12] != 0 and status[40] != 0          # inverted windows, a start beyond the row
        assert want[4].cpu().numpy().sum() == len(status) + 7 * sum(range(eng.nY + 1))     # incremented, not overwritten
    else:
        assert status[4] == 5 and (status[[0, 1, 2, 3]] == 0).all()             # 16 385 samples: beyond the plain limit


@pytest.mark.parametrize("slice_reads", [4, 0], ids=["slices-of-4", "built-in-slice"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_long_window_option_is_honoured(layout, slice_reads):
    """WDX_OPT_LONG_WINDOWS on the context: the 16 385-sample read and a 40 000-sample window are fingerprinted by both"""
    eng, b = _engine("long"), _batch("long40k")
    want = _float32_demux("long", "long40k")
    status = want[0].cpu().numpy()
    assert status[4] == 0 and status[-1] == 0 and (status[:4] == 0).all()
    shard, a_s, a_e = _shard(b, layout)
    with _slices(eng, slice_reads):
        got = _demux_outputs(eng, shard, a_s, a_e, None, max_len=b["rows"].shape[1])
    _all_same(got, want, (layout, slice_reads))


def test_window_beyond_max_len_is_reported_like_the_twin():
    """a call whose max_len is shorter than some windows: those reads come back WDX_READ_FAIL_UNKNOWN from both, and the
    staging block holds rows of max_len + 8 samples only"""
    eng, b = _engine("pad0"), _batch("long")
    stride, max_len = b["rows"].shape[1], 6144
    want = _demux_outputs(eng, _d(b["rows"]), _d(b["a_s"]), _d(b["a_e"]), None, stride=stride, max_len=max_len)
    status = want[0].cpu().numpy()
    assert (status[b["row_len"] > max_len] == 5).all() and (status[b["row_len"] <= max_len] == 0).all()
    for layout in LAYOUTS:
        shard, a_s, a_e = _shard(b, layout)
        _all_same(_demux_outputs(eng, shard, a_s, a_e, None, max_len=max_len), want, layout)
    assert eng.adc_staging_bytes(len(status), max_len) == len(status) * ((max_len + 8) * 4 + 12)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_refine_entries_equal_their_float32_twins(layout):
    """fingerprint_refine and demux_refine on the tRNA inputs, refine_idx included; three slices of 40 reads, then the built-in"""
    import torch

    eng, b = _engine("refine"), _batch("refine101")
    hr = sig_proc.RefineParams(query=ri.consensus(), **ri.REF)
    stride = b["rows"].shape[1]
    rows, ok = _d(b["rows"]), _d(b["ok"])

    def run(sig, a_s, a_e, **kw):
        fr = eng.fingerprint_refine(sig, a_s, a_e, hr, ok=ok, **kw)
        counts = torch.full((eng.nY + 1,), 3, dtype=torch.int64, device=eng.tdev)
        res, dwell, stats, idx = eng.demux_refine(sig, a_s, a_e, hr, ok=ok, counts=counts, **kw)
        torch.cuda.synchronize()
        return (*fr, res.status, res.fpt, res.dist, res.call, res.counts, dwell, stats, idx)

    want = run(rows, _d(b["a_s"]), _d(b["a_e"]), stride=stride, max_len=stride)
    ri.check_kinds(want[4].cpu().numpy(), False)
    assert (want[3].cpu().numpy()[want[4].cpu().numpy() == 0] >= 0).all()
    shard, a_s, a_e = _shard(b, layout)
    for slice_reads in (40, 0):
        with _slices(eng, slice_reads):
            _all_same(run(shard, a_s, a_e, max_len=stride), want, (layout, slice_reads))


@functools.lru_cache(maxsize=None)
def _tail_engine():
    """an engine whose references are fingerprints of the batch itself, with a small SVM, MLP and boost model resident"""
    from warpdemux_amd.engine import DemuxEngine

    b = _batch("main")
    p = sig_proc.SegParams(barcode_num_events=K, padding=b["padding"])
    fb = sig_proc.fingerprint_batch(b["rows"], b["a_s"], b["a_e"], p, success=b["ok"])
    m = svm_ref.synth_model(4, seed=5, n_support=[3, 1, 4, 2], n_extra=6, thresholds=True, gamma=0.02)
    refs = np.ascontiguousarray(fb.fpt[fb.status == 0][:m.n_train]) + 0.01
    assert refs.shape == (m.n_train, K)
    eng = DemuxEngine(refs, 15, 0.1, p)
    eng.set_svm(m.to_dtw_svm(refs))
    est = mlp_ref.random_mlp(len(refs), (16,), 5, np.float32, "relu", seed=9)
    lm = {i: 3 * i + 1 for i in range(5)}
    eng.set_mlp(models.from_reference(mlp_ref.DTW_MLP(est, refs, lm, np.linspace(0.05, 0.3, 5), window=15, penalty=0.1)))
    bm = boost_ref.random_model(33, (0, 1, 6, 3), 4, K, seed=81)
    trees = [(f, bo, [bm.nan_treatment[i] == "AsTrue" for i in f], lv) for f, bo, lv in bm.trees]
    eng.set_boost(models.Fpt_Boost(trees, bm.n_features, bm.scale, bm.bias, {i: 2 * i + 1 for i in range(4)},
                                   np.array([0.05, 0.2, 0.1, 0.3])))
    return eng


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tail", ["svm", "svm-fused", "mlp", "boost"])
def test_classifier_tails_equal_their_float32_twins(tail, layout):
    """demux_svm (row blocks with the distances, and the fused form without), demux_mlp (with its non-finite counter) and the
    plain demux_boost: three slices of 100 reads, then the built-in slice"""
    import torch

    eng, b = _tail_engine(), _batch("main")
    stride = b["rows"].shape[1]
    ok = _d(b["ok"])

    def run(sig, a_s, a_e, **kw):
        if tail.startswith("svm"):
            out = eng.demux_svm(sig, a_s, a_e, ok=ok, want_dist=tail == "svm", want_fpt=True, **kw)
        elif tail == "mlp":
            cnt = torch.full((1,), 5, dtype=torch.int64, device=eng.tdev)
            out = (*eng.demux_mlp(sig, a_s, a_e, ok=ok, want_dist=True, want_fpt=True, block_rows=37, n_nonfinite=cnt, **kw), cnt)
        else:
            out = eng.demux_boost(sig, a_s, a_e, None, ok=ok, want_fpt=True, want_raw=True, **kw)
        torch.cuda.synchronize()
        return out

    want = run(_d(b["rows"]), _d(b["a_s"]), _d(b["a_e"]), stride=stride, max_len=stride)
    status, pred = want[3].cpu().numpy(), want[1].cpu().numpy()
    assert 0 < (status != 0).sum() < len(status) and (pred[status != 0] == -1).all()
    shard, a_s, a_e = _shard(b, layout)
    for slice_reads in (100, 0):
        with _slices(eng, slice_reads):
            _all_same(run(shard, a_s, a_e, max_len=stride), want, (tail, layout, slice_reads))


def test_boost_tail_behind_the_refinement_branch():
    import torch

    eng, b = _engine("refine"), _batch("refine101")
    hr = sig_proc.RefineParams(query=ri.consensus(), **ri.REF)
    bm = boost_ref.random_model(17, 6, 4, K, seed=82)
    trees = [(f, bo, [bm.nan_treatment[i] == "AsTrue" for i in f], lv) for f, bo, lv in bm.trees]
    eng.set_boost(models.Fpt_Boost(trees, bm.n_features, bm.scale, bm.bias, {i: i for i in range(4)}, None))
    stride = b["rows"].shape[1]
    want = eng.demux_boost(_d(b["rows"]), _d(b["a_s"]), _d(b["a_e"]), hr, stride=stride, max_len=stride, ok=_d(b["ok"]),
                           want_fpt=True, want_raw=True)
    torch.cuda.synchronize()
    assert want[4] is not None and (want[3].cpu().numpy() == 6).sum() >= 3
    for layout in LAYOUTS:
        shard, a_s, a_e = _shard(b, layout)
        with _slices(eng, 40):
            got = eng.demux_boost(shard, a_s, a_e, hr, max_len=stride, ok=_d(b["ok"]), want_fpt=True, want_raw=True)
            torch.cuda.synchronize()
        _all_same(got, want, layout)


def test_staging_block_is_reused_and_regrown_across_calls():
    """one context: a small call (10 reads, rows of 16 392 floats), a larger one (256 reads, rows of 9 008 floats: the block
    grows), the first again in the grown block, then the larger in slices of 100 (a smaller block would do) -- each the twin's"""
    eng = _engine("pad0")
    calls = [("long", 0), ("main", 0), ("long", 0), ("main", 100)]
    need = []
    for name, slice_reads in calls:
        b = _batch(name)
        stride = b["rows"].shape[1]
        # (the main batch under this engine's padding 0: another twin than the padding-100 one above)
        want = _demux_outputs(eng, _d(b["rows"]), _d(b["a_s"]), _d(b["a_e"]), _d(b["ok"]), stride=stride, max_len=stride)
        shard, a_s, a_e = _shard(b, "strided")
        with _slices(eng, slice_reads):
            need.append(eng.adc_staging_bytes(len(b["a_s"]), stride))
            _all_same(_demux_outputs(eng, shard, a_s, a_e, _d(b["ok"]), max_len=stride), want, (name, slice_reads))
    assert need[0] < need[1] and need[3] < need[1]


def test_empty_shard_returns_success():
    import torch
    from warpdemux_amd.engine import AdcShard

    eng = _engine("pad100")
    e = lambda dt: torch.empty(0, dtype=dt, device=eng.tdev)   # noqa: E731
    for shard in (AdcShard(torch.empty((0, 64), dtype=torch.int16, device=eng.tdev), e(torch.int32), e(torch.float32), e(torch.float32)),
                  AdcShard(e(torch.int16), e(torch.int32), e(torch.float32), e(torch.float32),
                           offsets=torch.zeros(1, dtype=torch.int64, device=eng.tdev))):
        r = eng.demux(shard, e(torch.int32), e(torch.int32), max_len=64, want_fpt=True)
        fpt, dwell, stats, status = eng.fingerprint(shard, e(torch.int32), e(torch.int32), max_len=64)
        torch.cuda.synchronize()
        assert r.dist.shape == (0, eng.nY) and r.counts.cpu().numpy().sum() == 0 and status.shape == (0,)
    assert eng.adc_staging_bytes(0, 64) == 0
    with pytest.raises(ValueError, match="carries its own"):
        eng.demux(shard, e(torch.int32), e(torch.int32), max_len=64, stride=64)


def test_adcshard_refuses_tensors_that_do_not_cover_its_reads():
    """what the shapes can show is checked on the host, before any kernel reads through them"""
    import torch
    from warpdemux_amd.engine import AdcShard

    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")   # noqa: E731
    rl, off, sc = z(4, torch.int32), z(4, torch.float32), z(4, torch.float32)
    AdcShard(z((4, 64), torch.int16), rl, off, sc)
    AdcShard(z(256, torch.int16), rl, off, sc, stride=64)
    AdcShard(z(64, torch.int16), rl, off, sc, offsets=torch.tensor([0, 16, 32, 48, 64], device="cuda"))
    with pytest.raises(ValueError, match="one row of `stride` samples per read"):
        AdcShard(z((3, 64), torch.int16), rl, off, sc)
    with pytest.raises(ValueError, match="one row of `stride` samples per read"):
        AdcShard(z((4, 64), torch.int16), rl, off, sc, stride=128)
    with pytest.raises(ValueError, match="need more"):
        AdcShard(z(255, torch.int16), rl, off, sc, stride=64)
    with pytest.raises(ValueError, match="last offset"):
        AdcShard(z(56, torch.int16), rl, off, sc, offsets=torch.tensor([0, 16, 32, 48, 64], device="cuda"))
    with pytest.raises(ValueError, match="one entry per read"):
        AdcShard(z((4, 64), torch.int16), rl, off[:3].contiguous(), sc)


def test_plain_boost_call_sizes_its_workspace_by_the_plain_branch():
    """demux_boost without `refine` on a shard is planned by WDX_OPT_LONG_WINDOWS alone: with only the refinement option on and
    max_len beyond 16 384, its workspace is the plain twin's (wdx_demux_adc_workspace_bytes), and the results are the twin's"""
    import torch
    from warpdemux_amd.engine import DemuxEngine

    b = _batch("main")
    eng = DemuxEngine(np.random.default_rng(8).normal(size=(10, K)), 15, 0.1, sig_proc.SegParams(barcode_num_events=K, padding=100))
    try:
        eng.ctx.set_option(_lib.OPT_LONG_REFINE_WINDOWS, 1)
        bm = boost_ref.random_model(9, 3, 4, K, seed=83)
        trees = [(f, bo, [bm.nan_treatment[i] == "AsTrue" for i in f], lv) for f, bo, lv in bm.trees]
        eng.set_boost(models.Fpt_Boost(trees, bm.n_features, bm.scale, bm.bias, {i: i for i in range(4)}, None))
        stride, n, max_len = b["rows"].shape[1], len(b["a_s"]), 40000
        want = eng.demux_boost(_d(b["rows"]), _d(b["a_s"]), _d(b["a_e"]), None, stride=stride, max_len=max_len, ok=_d(b["ok"]),
                               want_fpt=True, want_raw=True)
        torch.cuda.synchronize()
        eng._refine_work = None
        shard, a_s, a_e = _shard(b, "strided")
        with _slices(eng, 100):
            got = eng.demux_boost(shard, a_s, a_e, None, max_len=max_len, ok=_d(b["ok"]), want_fpt=True, want_raw=True)
            torch.cuda.synchronize()
            plain = eng.L.wdx_demux_adc_workspace_bytes(eng.ctx.handle, n, max_len, K)
        assert eng._work.numel() >= plain > 0 and eng._refine_work is None
        # the plain branch stages rows of the plain limit, the refining one of max_len: two plans, and the call took the first
        assert eng.adc_staging_bytes(n, max_len, refine=False) < eng.adc_staging_bytes(n, max_len, refine=True)
        _all_same(got, want, "plain boost")
    finally:
        eng.close()
