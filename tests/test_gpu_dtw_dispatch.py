"""Every DTW kernel, operand layout and dispatch edge by name, against the oracle.

The DTW stage has seven kernel instantiations (wavefront, short<25,15>, band<8>, band<15> (EXACT_W), band<16>, band<32>,
scratch rows; plus short+svm, tests/test_gpu_svm.py) and three operand layouts behind one dispatcher.  Every case here
first asks the library which of them it ran (wdx_dtw_last_launch) -- the thresholds between the routes are tuning
constants -- and then compares float32 distances bit for bit with oracle.wdx_oracle.dtw_matrix and the argmin with
orc.argmin_rows / np.argmin, NaN rows included (test_gpu_parity._check_dist; no tolerance).

Cases too large for the oracle pair by pair are checked twice: (a) the oracle on a fixed row subset (first two waves,
last wave, 128 rows around every launch boundary, 2 000 drawn rows) and (b) EVERY row against a second device route that
the small cases pin to the oracle: the same rows through the read-minor form in chunks of 4 096."""
import numpy as np
import pytest

from oracle import wdx_oracle as orc
from warpdemux_amd import _lib, parallel_distances as pdist, sig_proc
from helpers.dtw_cases import (RL, RM, TM, effective_window, equal_infinities, fused_rule, instantiation, kernel_of, last_route,
                               nonfinite_reads, nonfinite_refs, options, oracle_dtw, read_minor_in_chunks, subset_rows)
from test_gpu_parity import _check_dist, _same

pytestmark = pytest.mark.gpu

PENALTIES = (None, 0.0, 0.1, 1.5)


def _check(X, Y, w, p, kernel, fused=None, launches=1):
    """nearest_reference on the route `kernel` = (family, W, EXACT_W, layout) against the oracle; returns the route."""
    got, am = pdist.nearest_reference(X, Y, w, p)
    r = last_route()
    assert kernel_of(r) == kernel, (r, kernel)
    assert r.launches == launches and r.window == effective_window(w, X.shape[1]), r
    if r.family in ("band", "short") and r.layout != RL:
        assert r.grid_x == (X.shape[0] + 63) // 64, r
    if fused is not None:
        assert r.fused == fused, r
    ref = oracle_dtw(X, Y, w, p)
    _check_dist(got, ref)
    assert np.array_equal(am, orc.argmin_rows(ref))
    assert np.array_equal(am, np.argmin(ref, axis=1))
    return r


# ------------------------------------------------------------------------- band<8>, <16>, <32>, <15> ----

def _lengths(w):
    return sorted({L for L in (1, 2, w - 1, w, w + 1, 2 * w - 2, 2 * w - 1, 2 * w, 25, 110, 257) if L >= 1})


@pytest.mark.parametrize("w", range(1, 33))
def test_band_kernels_every_window_at_the_lengths_where_the_band_leaves_the_matrix(w):
    """Read-minor band kernels (65 reads: a full and a partial wave, ld = 128) for every window 1..32, lengths either
    side of w and 2w - 1 (the band's head and tail rows overlap, meet, separate), 25, 110 and 257 (beyond the wavefront
    kernel), four penalties.  L < w makes the effective window L: the instantiation follows it."""
    rng = np.random.default_rng(100 + w)
    with options(no_wavefront=1, no_short=1):
        for L in _lengths(w):
            X, Y = rng.normal(size=(65, L)), rng.normal(size=(3, L))
            fam = instantiation(w, L, short=False)
            assert fam[0] == "band"
            for p in PENALTIES:
                _check(X, Y, w, p, fam + (TM,), fused=False)


@pytest.mark.parametrize("L", [1, 2, 7, 8, 9, 14, 15, 16, 17, 31, 32])
def test_band_kernels_unbanded_short_series(L):
    """window None / 0 / L / L + 3 with L <= 32: the effective window is L (band<8> up to 8, <16>, <15> at 15, <32>)."""
    rng = np.random.default_rng(200 + L)
    X, Y = rng.normal(size=(130, L)), rng.normal(size=(4, L))
    with options(no_wavefront=1):
        for w in (None, 0, L, L + 3):
            for p in (None, 0.1):
                r = _check(X, Y, w, p, instantiation(L, L) + (TM,), fused=False)
                assert r.window == L


@pytest.mark.parametrize("L", [1, 2, 13, 14, 15, 16, 27, 28, 29, 30, 31, 110])
def test_band15_read_minor_masked_branch_and_templates(L):
    """dtw_band_kernel<15, EXACT_W>: L < 28 takes the masked rows, L >= 28 the head / tail templates around a body of
    L - 28 rows (0, 1, 2, 3, 82).  L < 15 has effective window L and leaves this instantiation: asserted as such."""
    rng = np.random.default_rng(300 + L)
    X, Y = rng.normal(size=(129, L)), rng.normal(size=(5, L))
    with options(no_wavefront=1):
        for p in PENALTIES:
            _check(X, Y, 15, p, instantiation(15, L) + (TM,), fused=False)
    if L >= 15:
        assert instantiation(15, L) == ("band", 15, True)


@pytest.mark.parametrize("L", [28 + b for b in (0, 1, 7, 8, 9, 15, 16, 17, 23, 24)] + [110, 256, 300])
def test_band15_row_major_chunk_loop_remainders(L):
    """Row-major band<15>: the body rows are fetched eight at a time one chunk ahead; bodies of 0, 1, 7, 8, 9, 15, 16, 17,
    23, 24 rows (no chunk, one chunk exactly, every remainder side) and 110, 256, 300.  8 193 reads: every row against
    the oracle (the last wave holds one active lane: the al = nA - 1 clamp)."""
    rng = np.random.default_rng(400 + L)
    nX = 8193
    X, Y = rng.normal(size=(nX, L)), rng.normal(size=(2, L))
    with options(no_wavefront=1):
        r = _check(X, Y, 15, 0.1, ("band", 15, True, RM))
    assert r.grid_x == 129
    if L in (28, 37, 52, 110):
        D, am = read_minor_in_chunks(X, Y, 15, 0.1)
        got, am2 = pdist.nearest_reference(X, Y, 15, 0.1)
        assert _same(D, got) and np.array_equal(am, am2)


# ------------------------------------------------------------------------------------- short<25,15> ----

@pytest.mark.parametrize("nX,nY,layout", [(64, 300, TM), (65, 300, TM), (200, 7, TM), (1, 100, RL), (3, 200, RL), (63, 300, RL),
                                          (8192, 3, RM), (8193, 3, RM), (8255, 2, RM)])
def test_short_kernel_in_every_layout(nX, nY, layout):
    rng = np.random.default_rng(500 + nX)
    X, Y = rng.normal(size=(nX, 25)), rng.normal(size=(nY, 25))
    X[nX // 2] = Y[nY - 1]          # distance 0
    with options(no_wavefront=1):
        for p in (0.1, None):
            _check(X, Y, 15, p, ("short", 15, True, layout))
    with options(no_wavefront=1, no_short=1):   # the same shape on the masked EXACT_W rows of band<15> (L = 25 < 28)
        _check(X, Y, 15, 0.1, ("band", 15, True, layout))


def test_short_and_band_kernels_row_major_on_device_rows():
    """wdx_dtw_matrix_dev on row-major device fingerprints (no NaN flags from a transpose): dtw_short_kernel<25,15,true>
    flags its rows from the registers, the band kernels by the lazy sweep.  Every instantiation, NaN / inf rows, a whole
    wave of NaN rows, a wave with exactly one, references with NaN / an exact tie; product, six-operation and
    settle-everything modes."""
    import torch
    from warpdemux_amd.engine import DemuxEngine
    for w, L in ((15, 25), (15, 41), (5, 30), (12, 30), (20, 40)):
        rng = np.random.default_rng(600 + w + L)
        X = nonfinite_reads(rng, 8200, L)
        for Y in (nonfinite_refs(rng, L), nonfinite_refs(rng, L)[:4]):
            ref = oracle_dtw(X, Y, w, 0.1)
            eng = DemuxEngine(Y, w, 0.1, sig_proc.SegParams(barcode_num_events=L))
            Xd = torch.from_numpy(X).to(eng.tdev)
            for mode in (0, 1, 2):
                with options(eng.ctx, unfused=mode):
                    d, am = eng.dtw(Xd, want_argmin=True)
                    eng.ctx.synchronize()
                assert kernel_of(last_route(eng.ctx)) == instantiation(w, L) + (RM,)
                _check_dist(d.cpu().numpy(), ref)
                assert np.array_equal(am.cpu().numpy(), orc.argmin_rows(ref))
            del eng, Xd
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ layouts ----

BANDS = [(5, 40), (12, 40), (20, 33), (15, 40)]     # (window, L): band<8>, <16>, <32>, <15>


@pytest.mark.parametrize("w,L", BANDS)
@pytest.mark.parametrize("nX", [64, 65, 127, 128, 8191])
def test_band_kernels_read_minor(nX, w, L):
    """ld = round_up(nX, 64): full waves, one lane in the last wave, one lane missing, the largest read-minor batch"""
    rng = np.random.default_rng(700 + nX + w)
    X, Y = rng.normal(size=(nX, L)), rng.normal(size=(2, L))
    with options(no_wavefront=1):
        r = _check(X, Y, w, 0.1, instantiation(w, L) + (TM,))
    assert r.grid_x == (nX + 63) // 64


@pytest.mark.parametrize("w,L", BANDS)
@pytest.mark.parametrize("nX", [8192, 8193, 8255])
def test_band_kernels_row_major(nX, w, L):
    """a lane reads its own row; the inactive lanes of the last wave are clamped to row nA - 1"""
    rng = np.random.default_rng(800 + nX + w)
    X, Y = rng.normal(size=(nX, L)), rng.normal(size=(2, L))
    with options(no_wavefront=1):     # (8 192 x 2 pairs are still the wavefront kernel's)
        r = _check(X, Y, w, None, instantiation(w, L) + (RM,))
        got, am2 = pdist.nearest_reference(X, Y, w, None)
    assert r.grid_x == (nX + 63) // 64
    D, am = read_minor_in_chunks(X, Y, w, None)
    assert _same(D, got) and np.array_equal(am, am2)


@pytest.mark.parametrize("w,L", BANDS)
@pytest.mark.parametrize("nX,nY", [(1, 70), (2, 129), (63, 64), (63, 300)])
def test_band_kernels_refs_as_lanes(nX, nY, w, L):
    """few reads, more references: the lanes run over the resident transposed references (out strides 1, nY)"""
    rng = np.random.default_rng(900 + nX + w)
    X, Y = rng.normal(size=(nX, L)), rng.normal(size=(nY, L))
    Y[nY - 1] = Y[0]
    with options(no_wavefront=1):
        r = _check(X, Y, w, 0.1, instantiation(w, L) + (RL,), fused=False)
    assert r.grid_x == (nY + 63) // 64


def test_wavefront_switch_changes_the_route_only():
    rng = np.random.default_rng(12)
    X, Y = rng.normal(size=(70, 110)), rng.normal(size=(9, 110))
    a = pdist.distance_matrix_to(X, Y, window=8, penalty=0.1, n_jobs=1)
    assert kernel_of(last_route()) == ("wavefront", 0, False, RM)
    with options(no_wavefront=1):
        b = pdist.distance_matrix_to(X, Y, window=8, penalty=0.1, n_jobs=1)
        assert kernel_of(last_route()) == ("band", 8, False, TM)
    assert _same(a, b)
    _check_dist(a, orc.dtw_matrix(X, Y, 8, 0.1))


# ------------------------------------------------------------------------------------- scratch rows ----

@pytest.mark.parametrize("L", [33, 34, 110, 200])
def test_scratch_kernel_windows_and_layouts(L):
    """Effective windows beyond 32: w = 33, L - 1, L, None; 1 / 63 / 64 / 65 reads against one reference (read-minor) and
    1 / 63 reads against more references than reads (refs-as-lanes: lanes over the references, out strides 1, nY).  The
    argmin comes from the separate kernel (the scratch path has no fused form)."""
    rng = np.random.default_rng(1000 + L)
    for w in (33, L - 1, L, None):
        if effective_window(w, L) <= 32:
            continue
        for nX, nY, layout in ((1, 1, TM), (63, 2, TM), (64, 2, TM), (65, 3, TM), (1, 66, RL), (63, 65, RL)):
            X, Y = rng.normal(size=(nX, L)), rng.normal(size=(nY, L))
            Y[nY - 1] = Y[0]
            for p in ((0.1, None) if L < 110 else (0.1,)):
                _check(X, Y, w, p, ("scratch", 0, False, layout), fused=False)
    X = nonfinite_reads(rng, 200, L)
    for Y in (nonfinite_refs(rng, L), nonfinite_refs(rng, L)[:4]):
        _check(X, Y, None, 0.1, ("scratch", 0, False, TM), fused=False)
        _check(X[:5], np.vstack([Y, Y, Y]), None, 0.1, ("scratch", 0, False, RL), fused=False)


@pytest.mark.parametrize("nX,launches", [(65536, 1), (65537, 2), (131073, 3)])
def test_scratch_kernel_launch_loop(nX, launches):
    """One launch per 65 536 lanes (the scratch rows are that wide): either side of the step and a third launch holding one
    lane.  A batch this large would be row-major with a fused argmin on the band kernels; here the dispatcher keeps the
    read-minor copy and the separate argmin."""
    L, w, p = 34, 33, 0.1
    rng = np.random.default_rng(nX)
    Y = rng.normal(size=(3, L))
    Y[2] = Y[0]
    X = Y[rng.integers(0, 2, nX)] + rng.normal(size=(nX, L))
    X[65535, 3] = np.nan
    X[nX - 1, L - 1] = np.inf
    got, am = pdist.nearest_reference(X, Y, w, p)
    r = last_route()
    assert kernel_of(r) == ("scratch", 0, False, TM) and r.launches == launches and not r.fused, r
    sub = subset_rows(nX, boundaries=(65536, 131072), seed=nX)
    ref = oracle_dtw(X[sub], Y, w, p)
    _check_dist(got[sub], ref)
    assert np.array_equal(am[sub], orc.argmin_rows(ref))
    D, am2 = read_minor_in_chunks(X, Y, w, p)
    assert _same(D, got) and np.array_equal(am, am2)
    assert np.array_equal(am, orc.argmin_rows(got))


# --------------------------------------------------------------------------- grid split, fused argmin ----

GRID_SHAPES = [(16, 8), (25, 15), (40, 15), (30, 12), (40, 20)]    # band<8>, short, band<15>, band<16>, band<32>


@pytest.mark.parametrize("L,w", GRID_SHAPES)
def test_reference_split_over_grid_y_and_the_argmin(L, w):
    """Few waves of reads: the references are split over grid.y (`rpb` per block, the last block takes the remainder) and
    the argmin is a second kernel -- except for a single reference.  Duplicated references (exact ties -> lowest index)
    in different blocks; then a NaN reference, which wins every row."""
    rng = np.random.default_rng(1100 + L)
    remainders = 0
    cases = [(130, nY) for nY in (1, 15, 16, 17, 31, 32, 33, 100, 851, 1368)]
    if (L, w) == (16, 8):
        cases += [(1500, nY) for nY in (100, 851, 1368)]    # (more waves of reads: larger reference blocks)
    for nX, nY in cases:
        X = rng.normal(size=(nX, L))
        Y = rng.normal(size=(nY, L))
        Y[nY - 1] = Y[0]
        if nY > 40:
            Y[37] = Y[0]
        X[7] = Y[nY // 2]
        with options(no_wavefront=1):
            r = _check(X, Y, w, 0.1, instantiation(w, L) + (TM,), fused=fused_rule(nX, nY))
            assert r.fused == (nY == 1)
            remainders += nY % r.rpb != 0
            if nY >= 17:
                Y[nY - 2, L // 2] = np.nan
                _check(X, Y, w, 0.1, instantiation(w, L) + (TM,), fused=False)
    assert remainders >= (3 if (L, w) == (16, 8) else 1), "no case left a partial last block of references"


def _large(nX, nY, L, w, p, seed, kernel, fused):
    """a large row-major case: (a) oracle on the fixed subset, (b) every row against the read-minor route"""
    rng = np.random.default_rng(seed)
    Y = rng.normal(size=(nY, L))
    Y[nY - 1] = Y[1 % nY]                                     # exact tie: the lower index wins
    X = Y[rng.integers(0, nY, nX)] + 0.7 * rng.normal(size=(nX, L))
    X[nX - 1] = Y[nY - 1]
    got, am = pdist.nearest_reference(X, Y, w, p)
    r = last_route()
    assert kernel_of(r) == kernel and r.fused == fused == fused_rule(nX, nY) and r.grid_x == (nX + 63) // 64, r
    if fused:
        assert r.grid_y == 1 and r.rpb == nY, r
    sub = subset_rows(nX, seed=seed)
    ref = oracle_dtw(X[sub], Y, w, p)
    _check_dist(got[sub], ref)
    assert np.array_equal(am[sub], orc.argmin_rows(ref))
    D, am2 = read_minor_in_chunks(X, Y, w, p)
    assert _same(D, got), np.count_nonzero(D != got)
    assert np.array_equal(am, am2) and np.array_equal(am, orc.argmin_rows(got))
    assert am[nX - 1] == 1 % nY
    return X, Y, got


@pytest.mark.parametrize("nX", [131008, 131009])
@pytest.mark.parametrize("nY", [31, 32])
def test_fused_argmin_either_side_of_2048_waves(nX, nY):
    """gx = 2047 / 2048 with 31 / 32 references: the argmin is folded into the band kernel only at gx >= 2048 and fewer than
    32 references"""
    _large(nX, nY, 16, 8, 0.1, nX + nY, ("band", 8, False, RM), fused=(nX == 131009 and nY == 31))


@pytest.mark.parametrize("L,w,nY", [(25, 15, 10), (30, 15, 10), (30, 12, 4), (40, 20, 3)])
def test_fused_argmin_on_the_other_instantiations(L, w, nY):
    """short, band<15>, band<16>, band<32> row-major with the argmin in the kernel; then with a NaN reference column"""
    nX = 131_100
    X, Y, _ = _large(nX, nY, L, w, 0.1, 1300 + L + w, instantiation(w, L) + (RM,), fused=True)
    Y[nY - 2, 0] = np.nan
    got, am = pdist.nearest_reference(X[:70_000], Y, w, 0.1)
    assert not last_route().fused                              # (gx < 2048: the separate kernel, same answer)
    got2, am2 = pdist.nearest_reference(X, Y, w, 0.1)
    assert last_route().fused
    assert (am2 == nY - 2).all() and (am == nY - 2).all() and np.isnan(got2[:, nY - 2]).all()
    assert _same(got2[:70_000], got)
    sub = subset_rows(nX, seed=5, drawn=500)
    _check_dist(got2[sub], oracle_dtw(X[sub], Y, w, 0.1))


def test_fused_argmin_above_24576_waves_with_many_references():
    """gx >= 8 * 3072: one block walks all 32 references and folds the argmin in, whatever their number"""
    _large(64 * 8 * 3072 + 1, 32, 16, 8, 0.1, 77, ("band", 8, False, RM), fused=True)


# ---------------------------------------------------------------------- non-finite and extreme values ----

@pytest.mark.parametrize("w,L", BANDS + [(15, 25), (15, 110), (3, 257)])
def test_nonfinite_values_on_every_instantiation_and_layout(w, L):
    """NaN at the first / a middle / the last sample of a read and of a reference, reads with +inf, -inf, both in one row,
    inf next to NaN and nothing but +inf, a whole wave of NaN rows and a wave with exactly one.
    Read-minor (the transpose's flags), row-major (the lazy sweep: host rows reach the kernel without flags, too) and
    refs-as-lanes (the flags swap sides), in the product, six-operation and settle-everything modes; with the NaN
    references (they win every row) and without (ties, infinities decide)."""
    rng = np.random.default_rng(1400 + w + L)
    fam = instantiation(w, L)
    Xs = {TM: nonfinite_reads(rng, 200, L), RM: nonfinite_reads(rng, 8200 if L <= 110 else 8193, L)}
    for extra in (0, 60):
        Yn = nonfinite_refs(rng, L, extra)
        for Y in (Yn, np.delete(Yn, (4, 5, 6), axis=0)):
            cases = [(Xs[TM], Y, TM), (Xs[RM], Y, RM)] if extra == 0 else [(Xs[TM][:9], Y, RL)]
            for X, Yv, layout in cases:
                ref = oracle_dtw(X, Yv, w, 0.1)
                for mode in (0, 1, 2):
                    with options(no_wavefront=1, unfused=mode):
                        got, am = pdist.nearest_reference(X, Yv, w, 0.1)
                    assert kernel_of(last_route()) == fam + (layout,), last_route()
                    _check_dist(got, ref)
                    assert np.array_equal(am, orc.argmin_rows(ref)) and np.array_equal(am, np.argmin(ref, axis=1))
                nanrow = np.isnan(X).any(axis=1)
                assert np.array_equal(np.isnan(got).all(axis=1), nanrow)


@pytest.mark.parametrize("w,L", BANDS + [(15, 25)])
def test_scaled_inputs_reach_overflow_and_the_underflow_guard(w, L):
    """d * d overflows (1e160), the accumulated cost leaves [1e-280, 1e280] (dtw_unsettled's guard: 1e-150 and below,
    1e139 and above), squares underflow to zero (1e-170): read-minor, row-major (8 193 rows) and refs-as-lanes (9 reads x
    70 references), every scale in each, in the product, six-operation and settle-everything modes"""
    rng = np.random.default_rng(1500 + w + L)
    for nX, nY, layout in ((200, 4, TM), (8193, 4, RM), (9, 70, RL)):
        X, Y = rng.normal(size=(nX, L)), rng.normal(size=(nY, L))
        for scale in (1e-170, 1e-160, 1e-150, 1e-139, 1e139, 1e150, 1e160):
            p = 0.1 if scale > 1 else 0.0
            ref = oracle_dtw(X * scale, Y * scale, w, p)
            for mode in (0, 1, 2):
                with options(no_wavefront=1, unfused=mode):
                    got, am = pdist.nearest_reference(X * scale, Y * scale, w, p)
                assert kernel_of(last_route()) == instantiation(w, L) + (layout,)
                _check_dist(got, ref)
                assert np.array_equal(am, orc.argmin_rows(ref))


ALL_KERNELS = BANDS + [(15, 25), (33, 40), (None, 60)]     # band<8/16/32/15>, short, scratch (banded, unbanded)


@pytest.mark.parametrize("w,L", ALL_KERNELS)
def test_equal_infinities_in_read_and_reference(w, L):
    """+inf / +inf and -inf / -inf at the same index k = 0, L // 2, L - 1 of a read and a reference (inf - inf = NaN inside
    cell (k, k), no NaN sample), and +inf / +inf off the diagonal: the reference returns NaN for the former (a NaN diagonal
    predecessor survives its `if (t < minv)`), +inf for the latter.  v_min_f64 drops a NaN, so the DTW kernels alone return
    +inf for both; the dispatcher settles the former behind the kernel whenever a reference holds an infinity
    (launch_dtw_equal_inf) and takes the argmin again.  Every family in every layout it has, the wavefront kernel
    included, modes 0, 1, 2, against the oracle's bits and argmin."""
    rng = np.random.default_rng(1600 + L + (w or 0))
    fam = instantiation(w, L)
    shapes = [(200, 0, TM), (9, 61, RL)] + ([(8200, 0, RM)] if fam[0] != "scratch" else [])
    for nX, extra, layout in shapes:
        X, Y = equal_infinities(rng, nX, L, extra)
        ref = oracle_dtw(X, Y, w, 0.1)
        assert all(np.isnan(ref[k, k]) for k in range(1, 7)) and np.isinf(ref[7, 7]) and np.isnan(ref[8, 2]) and np.isnan(ref[8, 4])
        assert np.isinf(ref[1, 2]) and np.isinf(ref[1, 4]) and np.isfinite(ref[0, 0]) and np.isnan(ref[nX - 1, 2])
        for mode in (0, 1, 2):
            with options(no_wavefront=1, unfused=mode):
                got, am = pdist.nearest_reference(X, Y, w, 0.1)
                assert kernel_of(last_route()) == fam + (layout,), last_route()
                _check_dist(got, ref)
                assert np.array_equal(am, orc.argmin_rows(ref)) and np.array_equal(am, np.argmin(ref, axis=1))
                _check_dist(pdist.distance_matrix_to(X, Y, window=w, penalty=0.1, n_jobs=1), ref)
        if effective_window(w, L) <= 16:
            got, am = pdist.nearest_reference(X[:200], Y, w, 0.1)
            assert last_route().family == "wavefront"
            _check_dist(got, ref[:200])
            assert np.array_equal(am, orc.argmin_rows(ref[:200]))


def test_equal_infinities_on_device_rows():
    """the same through wdx_dtw_matrix_dev (row-major device rows, fused argmin asked for) on short and band<8>"""
    import torch
    from warpdemux_amd.engine import DemuxEngine
    for w, L in ((15, 25), (5, 40)):
        X, Y = equal_infinities(np.random.default_rng(1700 + L), 8200, L)
        ref = oracle_dtw(X, Y, w, 0.1)
        eng = DemuxEngine(Y, w, 0.1, sig_proc.SegParams(barcode_num_events=L))
        d, am = eng.dtw(torch.from_numpy(X).to(eng.tdev), want_argmin=True)
        eng.ctx.synchronize()
        assert kernel_of(last_route(eng.ctx)) == instantiation(w, L) + (RM,)
        _check_dist(d.cpu().numpy(), ref)
        assert np.array_equal(am.cpu().numpy(), orc.argmin_rows(ref))
        del eng
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------- route census ----

CENSUS = [   # (test of tests/test_gpu_parity.py, nX, nY, L, window)
    ("dtw_lengths L=1", 65, 5, 1, 15), ("dtw_lengths L=28", 65, 5, 28, 15), ("dtw_lengths L=200", 65, 5, 200, 15),
    ("dtw_windows w=5 L=110", 70, 9, 110, 5), ("dtw_windows w=16 L=110", 70, 9, 110, 16), ("dtw_windows w=17 L=110", 70, 9, 110, 17),
    ("dtw_windows w=None L=25", 70, 9, 25, None), ("dtw_windows w=32 L=110", 70, 9, 110, 32), ("dtw_windows w=33 L=110", 70, 9, 110, 33),
    ("dtw_nan_inf_and_ties", 130, 10, 110, 15),
    ("dtw_matrix_regimes 1000x10", 1000, 10, 110, 15), ("dtw_matrix_regimes 300x851", 300, 851, 25, 15),
    ("dtw_matrix_regimes 64x6", 64, 6, 110, 15), ("dtw_matrix_regimes 5000x10", 5000, 10, 110, 15),
    ("dtw_few_reads_many_refs nX=3", 3, 1368, 25, 15), ("dtw_few_reads_many_refs nX=63", 63, 1368, 25, 15),
    ("dtw_few_reads_many_refs nX=65", 65, 1368, 25, 15),
    ("dtw_large_batch_fused_argmin", 140_000, 10, 110, 15), ("fused_cells g10 L=25", 3000, 64, 25, 15),
    ("fused_cells g10 L=110", 20000, 64, 110, 15), ("lazy sweep shape (host rows)", 40_000, 10, 110, 15),
    ("kkt shape L=25 (host rows)", 2000, 10, 25, 15),
]


@pytest.mark.parametrize("name,nX,nY,L,w", CENSUS, ids=[c[0].replace(" ", "_").replace("(", "").replace(")", "") for c in CENSUS])
def test_route_census_of_the_parity_suite(name, nX, nY, L, w, capsys):
    """Replays the shapes of tests/test_gpu_parity.py's DTW tests and prints the route each takes, with and without the
    wavefront kernel, every shape as a host call (pytest -s shows the table; DESIGN.md 4.3 keeps the latest).  Asserted: the switch removes the
    wavefront kernel and nothing else, and the route is one the kernels' domains admit."""
    X, Y = np.zeros((nX, L)), np.ones((nY, L))
    rows = []
    for nowf in (0, 1):
        with options(no_wavefront=nowf):
            pdist.nearest_reference(X, Y, w, 0.1)
        rows.append(last_route())
    a, b = rows
    assert b.family != "wavefront" and (a == b or a.family == "wavefront")
    assert (b.family, b.band_w, b.exact_w) == instantiation(w, L)
    with capsys.disabled():
        for tag, r in (("default", a), ("no wavefront", b)):
            print("\nROUTE | %-32s | %6d x %-4d L=%-3d w=%-4s | %-12s | %-9s W=%-2d | %-13s | grid %5d x %-4d rpb %-4d | fused=%d launches=%d"
                  % (name, nX, nY, L, w, tag, r.family, r.band_w, r.layout, r.grid_x, r.grid_y, r.rpb, r.fused, r.launches), end="")
