"""Nearest-reference calls with reference labels, margin and rejection (wdx_nearest_dev, wdx_demux_nearest_dev, wdx_dtw_nearest)
on the GPU, route by route.

The reference of every comparison is tests/helpers/nearest_rule.py (the NumPy statement of the rule, pinned by hand-worked rows
in tests/test_nearest_host.py) applied to the float32 matrix `wdx_dtw_matrix_dev` returns for the same inputs on the same
context -- the distances themselves are pinned to the oracle by tests/test_gpu_dtw_dispatch.py and tests/test_gpu_wide_dtw.py.
`call`, `best` and `counts` must equal it bit for bit (NaN is 0x7fc00000 on both sides), `dist`, when asked for, the matrix.
Every case first asks the library which kernel family, layout and rule placement it took (wdx_dtw_last_launch; fused_argmin = 1:
the rule ran in the DTW kernel's epilogue, 0: nearest_rows_kernel ran on the matrix), so a changed dispatch cannot silently
skip a kernel."""
import numpy as np
import pytest

from warpdemux_amd import _lib, parallel_distances as pdist, sig_proc, synth
from helpers.dtw_cases import RL, RM, TM, last_route
from helpers.nearest_rule import QNAN, nearest_rule, same_bits

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _engine(L, wide=False):
    """one engine per fingerprint length and wide-window option for the whole module"""
    from warpdemux_amd.engine import DemuxEngine

    key = (L, bool(wide))
    if key not in _ENGINES:
        _ENGINES[key] = DemuxEngine(np.zeros((1, L)), 15, 0.1, sig_proc.SegParams(barcode_num_events=L), wide_dtw=bool(wide))
    return _ENGINES[key]


def _inputs(nX, nY, L, seed, refs="plain"):
    """Reads around the references, with the hard rows: references duplicated under one label (3 = 0) and under different labels
    (4 = 2; labels are c % 3), a read equal to reference 2 (d1 = 0, margin exactly 0, the call is column 2's label), a NaN
    read, reads with +inf / -inf samples; `refs`: "nan" / "inf" put such a sample into reference 1 (and the same infinity into
    read 4 at that index: the pair the settle pass turns into NaN)."""
    rng = np.random.default_rng(seed)
    Y = rng.normal(size=(nY, L))
    if nY >= 5:
        Y[3], Y[4] = Y[0], Y[2]
    X = Y[rng.integers(0, nY, size=nX)] + 0.4 * rng.normal(size=(nX, L))
    if nX > 8:
        X[1] = Y[min(2, nY - 1)]
        X[2, L // 2] = np.nan
        X[3, 0] = np.inf
        X[5, L - 1] = -np.inf
        X[6] = Y[0]
    if refs == "nan" and nY > 1:
        Y[1, 3] = np.nan
    if refs == "inf" and nY > 1:
        Y[1, 3] = np.inf
        if nX > 8:
            X[4, 3] = np.inf
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


def _status(nX, seed):
    st = np.zeros(nX, dtype=np.int32)
    if nX > 8:
        st[[7, nX - 1]] = [3, 1]
        st[np.random.default_rng(seed).integers(8, nX, size=max(1, nX // 50))] = 2   # (not the hard reads)
    return st


def _run(eng, X, Y, window, labels, G, *, want_dist, route=None, status=None, min_margin=None, max_dist=None, options=()):
    """`nearest` against the helper on wdx_dtw_matrix_dev's matrix; returns (result, helper's outputs, the matrix)"""
    import torch

    for opt, v in options:
        eng.ctx.set_option(opt, v)
    try:
        eng.set_refs(Y, window, 0.1)
        dX = torch.from_numpy(X).to(eng.tdev)
        D = eng.dtw(dX, want_argmin=False)[0]
        st = None if status is None else torch.from_numpy(status).to(eng.tdev)
        res = eng.nearest(dX, labels=labels, n_labels=G, min_margin=min_margin, max_dist=max_dist, want_dist=want_dist, status=st)
        r = last_route(eng.ctx)
        torch.cuda.synchronize()
    finally:
        for opt, _ in options:
            eng.ctx.set_option(opt, 0)
    if route is not None and X.shape[0] and Y.shape[0]:
        family, layout, fused = route
        assert (r.family, r.layout, r.fused) == (family, layout, fused), r
        if fused:
            assert r.grid_y == 1 and r.rpb == Y.shape[0], r
    D = D.cpu().numpy()
    want = nearest_rule(D, labels, G, min_margin, max_dist, status)
    call, best, counts = res.call.cpu().numpy(), res.best.cpu().numpy(), res.counts.cpu().numpy()
    assert np.array_equal(call, want[0]), np.flatnonzero(call != want[0])[:10]
    assert same_bits(best, want[1]), np.flatnonzero((best.view(np.uint32) != want[1].view(np.uint32)).any(axis=1))[:10]
    assert np.array_equal(counts, want[2]) and counts.sum() == X.shape[0]
    if want_dist:
        assert same_bits(res.dist.cpu().numpy(), D)
    else:
        assert res.dist is None
    return res, want, D


NO_WF = ((_lib.OPT_NO_WAVEFRONT_DTW, 1),)
# id: nX nY L window, engine's wide option, options of the call, (family, layout, rule fused)
ROUTES = {
    "short-rowmajor-fused": (131072, 6, 25, 15, False, (), ("short", RM, True)),
    "band8-fused": (131072, 6, 40, 8, False, (), ("band", RM, True)),
    "band15-fused": (131072, 6, 40, 15, False, (), ("band", RM, True)),
    "band16-fused": (131072, 6, 40, 16, False, (), ("band", RM, True)),
    "band32-fused": (131072, 6, 40, 32, False, (), ("band", RM, True)),
    "readminor-split": (4096, 6, 25, 15, False, (), ("short", TM, False)),
    "readminor-fused": (4096, 1, 25, 15, False, NO_WF, ("short", TM, True)),
    "readminor-band15-fused": (4096, 1, 40, 15, False, NO_WF, ("band", TM, True)),
    "gridy-split": (1000, 40, 33, 15, False, (), ("band", TM, False)),
    "refs-as-lanes": (8, 200, 25, 15, False, NO_WF, ("short", RL, False)),
    "wavefront": (16, 10, 25, 15, False, (), ("wavefront", RM, False)),
    "scratch": (300, 5, 40, None, False, (), ("scratch", TM, False)),
    "wide-split": (300, 5, 40, None, True, (), ("wide", TM, False)),
    "wide-rowmajor-fused": (131072, 5, 40, None, True, (), ("wide", RM, True)),
    "wide-readminor-fused": (4096, 1, 40, None, True, (), ("wide", TM, True)),
}


@pytest.mark.parametrize("want_dist", [True, False], ids=["dist", "nodist"])
@pytest.mark.parametrize("name", list(ROUTES))
def test_every_route_by_name(name, want_dist):
    """labels c % 3, a status array with failed reads, the hard reads of _inputs; with and without the distance output"""
    nX, nY, L, window, wide, options, route = ROUTES[name]
    X, Y = _inputs(nX, nY, L, seed=sum(map(ord, name)))
    labels = np.arange(nY, dtype=np.int32) % 3
    res, want, D = _run(_engine(L, wide), X, Y, window, labels, 3, want_dist=want_dist, route=route, status=_status(nX, 7),
                        options=options)
    if nX > 8 and nY >= 5:
        call, best = want[0], want[1]
        assert best[1, 0] == 0 and best[1, 1] == 0 and call[1] == 2      # equal to references 2 and 4: margin 0, column 2's label
        assert best[6, 0] == 0 and best[6, 1] > 0 and call[6] == 0       # equal to references 0 and 3, both label 0
        assert call[2] == -1 and np.isnan(best[2]).all()                  # the NaN read
        assert call[7] == -1 and np.isnan(best[7]).all()                  # status != 0
        assert np.isinf(D[3]).all() and call[3] == 0 and np.isinf(best[3]).all()   # an infinite sample: every distance +inf


@pytest.mark.parametrize("refs", ["nan", "inf"])
@pytest.mark.parametrize("name", [k for k in ROUTES if ROUTES[k][1] > 1])   # (the hard reference is reference 1)
def test_nan_and_infinite_references_on_every_route(name, refs):
    """A NaN reference makes every row hold a NaN (call -1, best NaN).  An infinite sample in a reference sends every route
    through the matrix (the pass that settles equal infinities rewrites it): the rule then runs behind the kernels."""
    nX, nY, L, window, wide, options, (family, layout, fused) = ROUTES[name]
    X, Y = _inputs(nX, nY, L, seed=11 + sum(map(ord, name)), refs=refs)
    route = (family, layout, fused and refs != "inf")
    res, want, D = _run(_engine(L, wide), X, Y, window, np.arange(nY, dtype=np.int32) % 3, 3, want_dist=False, route=route,
                        options=options)
    if refs == "nan":
        assert (want[0] == -1).all() and np.isnan(want[1]).all() and want[2][3] == nX
    elif nX > 8:
        assert np.isnan(D[4, 1]) and want[0][4] == -1     # equal infinities at one index: NaN, as the reference's DTW gives


@pytest.mark.parametrize("name", ["short-rowmajor-fused", "band15-fused", "gridy-split", "wavefront", "scratch", "wide-rowmajor-fused"])
def test_one_label_and_identity_labels(name):
    nX, nY, L, window, wide, options, route = ROUTES[name]
    eng = _engine(L, wide)
    X, Y = _inputs(nX, nY, L, seed=5)
    # G = 1: d2 is +inf on every row without a NaN
    res, want, D = _run(eng, X, Y, window, np.zeros(nY, dtype=np.int32), 1, want_dist=False, route=route, options=options)
    clean = ~np.isnan(D).any(axis=1)
    assert clean.sum() >= nX - 1 and np.isinf(want[1][clean, 1]).all() and (want[0][clean] == 0).all()
    # identity labels, no thresholds: the call is wdx_dtw_matrix_dev's argmin wherever the row has no NaN
    import torch

    res, want, D = _run(eng, X, Y, window, None, None, want_dist=True, route=route, options=options)
    for opt, v in options:
        eng.ctx.set_option(opt, v)
    am = eng.dtw(torch.from_numpy(X).to(eng.tdev))[1].cpu().numpy()
    for opt, _ in options:
        eng.ctx.set_option(opt, 0)
    assert np.array_equal(res.call.cpu().numpy()[clean], am[clean])


@pytest.mark.parametrize("nX", [0, 1, 65])
@pytest.mark.parametrize("options", [(), NO_WF], ids=["as-planned", "no-wavefront"])
@pytest.mark.parametrize("nY", [1, 6, 200])
def test_no_read_one_read_and_a_partial_second_wave(nX, nY, options):
    X, Y = _inputs(nX, nY, 25, seed=nX + nY)
    for want_dist in (True, False):
        res, want, _ = _run(_engine(25), X, Y, 15, np.arange(nY, dtype=np.int32) % 3, 3, want_dist=want_dist, options=options,
                            status=_status(nX, 3))
        assert res.call.shape == (nX,) and res.best.shape == (nX, 2) and res.counts.sum().item() == nX


@pytest.mark.parametrize("name", ["short-rowmajor-fused", "band15-fused", "gridy-split", "readminor-split", "wide-rowmajor-fused"])
def test_thresholds_flip_exactly_at_the_data_s_own_margins(name):
    """min_margin / max_dist per label = a margin / a nearest distance the data holds: exactly that value accepts the read, one
    float32 ulp further rejects it -- on the device as the helper says, for every read."""
    nX, nY, L, window, wide, options, route = ROUTES[name]
    eng = _engine(L, wide)
    X, Y = _inputs(nX, nY, L, seed=77)
    labels = np.arange(nY, dtype=np.int32) % 3
    _, (call, best, _), _ = _run(eng, X, Y, window, labels, 3, want_dist=False, route=route, options=options)
    rows, margin, d1 = [], np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        m_all = best[:, 1] - best[:, 0]
    for lab in range(3):
        # (margin 0 included: with 5 references label 2's only reference has a twin under label 1, so its reads all tie)
        idx = np.flatnonzero((call == lab) & np.isfinite(m_all))
        assert idx.size, "every label is some read's nearest"
        r = idx[np.argsort(m_all[idx])[idx.size // 2]]    # the median margin of the label's reads
        rows.append(r)
        margin[lab], d1[lab] = m_all[r], best[r, 0]
    rows = np.array(rows)
    inf = np.float32(np.inf)
    for thr, accepted in ((margin, True), (np.nextafter(margin, inf), False), (np.nextafter(margin, -inf), True)):
        res, want, _ = _run(eng, X, Y, window, labels, 3, want_dist=False, route=route, options=options, min_margin=thr)
        assert ((res.call.cpu().numpy()[rows] >= 0) == accepted).all()
    for thr, accepted in ((d1, True), (np.nextafter(d1, inf), True), (np.nextafter(d1, -inf), False)):
        res, want, _ = _run(eng, X, Y, window, labels, 3, want_dist=False, route=route, options=options, max_dist=thr,
                            min_margin=np.nextafter(margin, -inf))
        assert ((res.call.cpu().numpy()[rows] >= 0) == accepted).all()
    assert 0 < (want[0] >= 0).sum() < nX     # thresholds from the data reject some reads and keep others


# ---- the fused raw-row path ---------------------------------------------------------------------------------------------------
def test_demux_nearest_equals_demux_pushed_through_the_rule():
    """20 000 synthetic reads, K = 25, 12 references under 4 labels: wdx_demux_nearest_dev against wdx_demux_dev's dist and status
    through the helper; then with launch slices of 3 000 reads; and demux itself returns the same bits before and after."""
    import torch

    from warpdemux_amd.engine import DemuxEngine

    K, n, nY = 25, 20000, 12
    spec = synth.SynthSpec(n_barcodes=4)
    eng = DemuxEngine(np.zeros((nY, K)), 15, 0.1, sig_proc.SegParams(barcode_num_events=K))
    sig, off, a_s, a_e, bc, max_len = eng.synth_packed(spec, 0, n)
    fpt, _, _, st = eng.fingerprint(sig[: int(off[256].item())], a_s[:256], a_e[:256], offsets=off[:257], max_len=max_len, want_stats=False)
    good = np.flatnonzero(st.cpu().numpy() == 0)
    assert good.size >= nY
    refs = fpt.cpu().numpy()[good[:nY]]
    eng.set_refs(refs, 15, 0.1)
    labels = np.arange(nY, dtype=np.int32) % 4
    before = eng.demux(sig, a_s, a_e, offsets=off, max_len=max_len)
    torch.cuda.synchronize()
    D, status, call0 = before.dist.cpu().numpy(), before.status.cpu().numpy(), before.call.cpu().numpy()
    mm = np.full(4, np.float32(0.05))
    want = nearest_rule(D, labels, 4, mm, None, status)
    for max_slice, want_dist in ((0, False), (0, True), (3000, False)):
        eng.ctx.set_option(_lib.OPT_MAX_LAUNCH_SLICE, max_slice)
        try:
            res = eng.demux_nearest(sig, a_s, a_e, offsets=off, max_len=max_len, labels=labels, min_margin=mm, want_dist=want_dist)
            r = last_route(eng.ctx)
            torch.cuda.synchronize()
        finally:
            eng.ctx.set_option(_lib.OPT_MAX_LAUNCH_SLICE, 0)
        assert (r.family, r.layout, r.fused) == ("short", RM, False), r    # 313 waves of reads: the references are split
        assert np.array_equal(res.status.cpu().numpy(), status)
        assert np.array_equal(res.call.cpu().numpy(), want[0]) and same_bits(res.best.cpu().numpy(), want[1])
        counts = res.counts.cpu().numpy()
        assert np.array_equal(counts, want[2]) and counts.sum() == n and counts.shape == (5,)
        if want_dist:
            assert same_bits(res.dist.cpu().numpy(), D)
    assert 0 < (want[0] >= 0).sum() < n
    # a minibatch-sized call: below 8 192 reads the DTW reads a read-minor copy (kept in the context's own blocks here)
    m = 777
    small = eng.demux_nearest(sig[: int(off[m].item())], a_s[:m], a_e[:m], offsets=off[: m + 1], max_len=max_len, labels=labels,
                              min_margin=mm)
    r = last_route(eng.ctx)
    torch.cuda.synchronize()
    assert (r.family, r.layout, r.fused) == ("short", TM, False), r
    assert np.array_equal(small.call.cpu().numpy(), want[0][:m]) and same_bits(small.best.cpu().numpy(), want[1][:m])
    assert np.array_equal(small.status.cpu().numpy(), status[:m]) and small.counts.sum().item() == m
    # identity labels without thresholds: demux's own call
    res = eng.demux_nearest(sig, a_s, a_e, offsets=off, max_len=max_len)
    after = eng.demux(sig, a_s, a_e, offsets=off, max_len=max_len)
    torch.cuda.synchronize()
    assert np.array_equal(res.call.cpu().numpy(), call0) and np.array_equal(res.counts.cpu().numpy(), before.counts.cpu().numpy())
    # nothing else moved: demux on the same context gives the same bits after the new calls
    assert same_bits(after.dist.cpu().numpy(), D) and np.array_equal(after.call.cpu().numpy(), call0)
    assert np.array_equal(after.status.cpu().numpy(), status) and np.array_equal(after.counts.cpu().numpy(), before.counts.cpu().numpy())
    eng.close()


def test_demux_nearest_fused_rule_on_a_large_shard():
    """131 072 reads x 6 references: one lane walks every reference, so the rule runs in the DTW kernel behind the fingerprint
    stage and, without `dist`, no distance is written; same calls as demux's matrix through the helper."""
    import torch

    from warpdemux_amd.engine import DemuxEngine

    K, n, nY = 25, 131072, 6
    spec = synth.SynthSpec(n_barcodes=4)
    eng = DemuxEngine(np.zeros((nY, K)), 15, 0.1, sig_proc.SegParams(barcode_num_events=K))
    sig, off, a_s, a_e, bc, max_len = eng.synth_packed(spec, 0, n)
    fpt, _, _, st = eng.fingerprint(sig[: int(off[256].item())], a_s[:256], a_e[:256], offsets=off[:257], max_len=max_len, want_stats=False)
    good = np.flatnonzero(st.cpu().numpy() == 0)
    eng.set_refs(fpt.cpu().numpy()[good[:nY]], 15, 0.1)
    labels = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    ref = eng.demux(sig, a_s, a_e, offsets=off, max_len=max_len)
    res = eng.demux_nearest(sig, a_s, a_e, offsets=off, max_len=max_len, labels=labels, max_dist=np.float32(4.0))
    r = last_route(eng.ctx)
    torch.cuda.synchronize()
    assert (r.family, r.layout, r.fused) == ("short", RM, True), r
    want = nearest_rule(ref.dist.cpu().numpy(), labels, 3, None, np.float32(4.0), ref.status.cpu().numpy())
    assert np.array_equal(res.call.cpu().numpy(), want[0]) and same_bits(res.best.cpu().numpy(), want[1])
    assert np.array_equal(res.counts.cpu().numpy(), want[2]) and want[2].sum() == n
    eng.close()


# ---- the host seam ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nX,nY,L,G", [(1000, 10, 110, None), (200, 2601, 25, 11)], ids=["R1", "R2"])
def test_nearest_label_equals_distance_matrix_to_through_the_rule(nX, nY, L, G):
    X, Y = _inputs(nX, nY, L, seed=nY)
    labels = None if G is None else np.arange(nY) % G
    D = pdist.distance_matrix_to(X, Y, window=15, penalty=0.1, n_jobs=1)
    D0, am0 = pdist.nearest_reference(X, Y, 15, 0.1)
    want = nearest_rule(D, labels, G, np.float32(0.1), np.float32(6.0))
    call, best, dist = pdist.nearest_label(X, Y, labels, window=15, penalty=0.1, min_margin=0.1, max_dist=6.0, want_dist=True)
    assert np.array_equal(call, want[0]) and same_bits(best, want[1]) and same_bits(dist, D)
    call, best = pdist.nearest_label(X, Y, labels, window=15, penalty=0.1, min_margin=0.1, max_dist=6.0)
    assert np.array_equal(call, want[0]) and same_bits(best, want[1])
    assert 0 < (call >= 0).sum() < nX
    # nothing else moved: nearest_reference gives the same bits after the new calls on the default context
    D1, am1 = pdist.nearest_reference(X, Y, 15, 0.1)
    assert same_bits(D0, D1) and np.array_equal(am0, am1) and same_bits(D0, D)


def test_block_buffer_walks_several_row_blocks():
    """No `dist`, the rule behind the kernels, more rows than the 96 MiB block holds: 2 601 references are 9 664 rows per block;
    20 000 reads walk three blocks (the last one shorter, planned by its own size)."""
    nX, nY, L = 20000, 2601, 25
    rng = np.random.default_rng(3)
    Y = rng.normal(size=(nY, L))
    X = Y[rng.integers(0, nY, size=nX)] + 0.4 * rng.normal(size=(nX, L))
    labels = np.arange(nY) % 11
    call, best, dist = pdist.nearest_label(X, Y, labels, window=15, penalty=0.1, want_dist=True)
    want = nearest_rule(dist, labels, 11)
    assert np.array_equal(call, want[0]) and same_bits(best, want[1])
    call, best = pdist.nearest_label(X, Y, labels, window=15, penalty=0.1)
    r = last_route()
    assert r.family == "short" and not r.fused and r.grid_x == (nX - 2 * 9664 + 63) // 64, r
    assert np.array_equal(call, want[0]) and same_bits(best, want[1])


def test_refusals_leave_the_context_usable():
    import torch

    eng = _engine(25)
    X, Y = _inputs(100, 6, 25, seed=1)
    eng.set_refs(Y, 15, 0.1)
    dX = torch.from_numpy(X).to(eng.tdev)
    L, h, s = eng.L, eng.ctx.handle, eng._stream()
    call = torch.empty(100, dtype=torch.int32, device=eng.tdev)
    lab = torch.zeros(6, dtype=torch.int32, device=eng.tdev)
    p = lambda t: None if t is None else t.data_ptr()
    for labels, G in ((lab, 0), (lab, -3), (None, 5), (None, 7)):
        rc = L.wdx_nearest_dev(h, p(dX), 100, None, p(labels), G, None, None, None, p(call), None, None, s)
        assert rc == _lib.WDX_ERR_INVALID and L.wdx_last_error()
    with pytest.raises(ValueError):
        eng.nearest(dX, labels=[0, 1, 2, 3, 4, 9], n_labels=6)
    # device labels outside 0 .. G-1 (a documented precondition): a group of its own, called -1, nothing indexed out of bounds
    bad = torch.tensor([0, 1, 7, 0, -2, 1], dtype=torch.int32, device=eng.tdev)
    res = eng.nearest(dX, labels=bad, n_labels=2, min_margin=0.0, max_dist=100.0, want_dist=True)
    want = nearest_rule(res.dist.cpu().numpy(), bad.cpu().numpy(), 2, np.float32(0.0), np.float32(100.0))
    assert np.array_equal(res.call.cpu().numpy(), want[0]) and same_bits(res.best.cpu().numpy(), want[1])
    assert np.array_equal(res.counts.cpu().numpy(), want[2]) and (want[0] == -1).any()
    # no references resident: WDX_ERR_NO_REFS, from every entry
    ctx = _lib.Context(0)
    rc = L.wdx_nearest_dev(ctx.handle, p(dX), 100, None, p(lab), 1, None, None, None, p(call), None, None, s)
    assert rc == _lib.WDX_ERR_NO_REFS
    out = np.empty(100, dtype=np.int32), np.empty((100, 2), dtype=np.float32)
    rc = L.wdx_dtw_nearest(ctx.handle, _lib.ptr(X), 100, None, 6, None, None, None, _lib.ptr(out[0]), _lib.ptr(out[1]))
    assert rc == _lib.WDX_ERR_NO_REFS
    ctx.close()
    # a host label out of range is refused by the host entry itself
    pdist.nearest_label(X, Y, [0, 1, 2, 0, 1, 2])
    hl = np.array([0, 1, 2, 0, 1, 3], dtype=np.int32)
    rc = L.wdx_dtw_nearest(_lib.default_context().handle, _lib.ptr(X), 100, _lib.ptr(hl), 3, None, None, None, _lib.ptr(out[0]),
                           _lib.ptr(out[1]))
    assert rc == _lib.WDX_ERR_INVALID and b"label" in L.wdx_last_error()
    # ... and both contexts go on working
    _run(eng, X, Y, 15, np.arange(6, dtype=np.int32) % 3, 3, want_dist=False)
    call2, _ = pdist.nearest_label(X, Y, [0, 1, 2, 0, 1, 2])
    assert call2.shape == (100,)
