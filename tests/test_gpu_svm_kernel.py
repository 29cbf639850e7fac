"""The kernel matrix on the device (include/wdx.h: wdx_svm_kernel_device; DemuxEngine.svm_kernel) against the rule restated in NumPy
(tests/helpers/svm_cv_rule.py: kernel_matrix), bit for bit.

Shapes: m = 1 and 3 (less than one 16-byte access), 64 (whole accesses only), 257 (a ragged end) and 1 029 (a second run of
columns per row); ld = m (16-byte rows only where m is a multiple of four) and ld = m + 3 (never); in place and out of place;
p = 1, 2, 3.  Entries: 0, +inf, NaN, distances that leave float32's normal range after the exponential, and distances whose
exponent lies below -700 (exp_rule's zero branch)."""
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
from helpers import svm_cv_rule as cvr  # noqa: E402

pytestmark = pytest.mark.gpu


def _imports():
    global torch, _lib, DemuxEngine
    import torch
    from warpdemux_amd import _lib
    from warpdemux_amd.engine import DemuxEngine


@pytest.fixture(scope="module")
def eng():
    _imports()
    e = DemuxEngine(np.zeros((4, 25)), 15, 0.1)
    yield e
    e.close()


def _distances(m, seed):
    rng = np.random.default_rng(seed)
    D = rng.gamma(2.0, 4.0, size=(m, m)).astype(np.float32)
    flat = D.reshape(-1)
    special = np.array([0.0, np.inf, np.nan, 88.0, 95.0, 103.5, 104.0, 699.9, 700.1, 745.0, 1e4, 3e38, 1e-30, -0.0], np.float32)
    idx = rng.permutation(flat.size)[: min(flat.size, len(special))]
    flat[idx] = special[: len(idx)]
    return D


@pytest.mark.parametrize("m", [1, 3, 64, 257, 1029])
@pytest.mark.parametrize("pad", [0, 3])
def test_kernel_matrix_equals_the_rule(eng, m, pad):
    D = _distances(m, seed=m + pad)
    for p, gamma in ((1, 1.0), (2, 0.05), (3, 1e-3)):
        want = cvr.kernel_matrix(D, gamma, p)
        wide = torch.full((m, m + pad), -7.0, dtype=torch.float32, device="cuda")
        wide[:, :m] = torch.tensor(D)
        out = torch.full((m, m + pad), -9.0, dtype=torch.float32, device="cuda")
        got = eng.svm_kernel(wide[:, :m], gamma, p, out=out[:, :m])
        assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), (m, pad, p)
        assert (out[:, m:] == -9.0).all() and (wide[:, m:] == -7.0).all()           # the columns from m on are left alone
        assert np.array_equal(wide[:, :m].cpu().numpy(), D, equal_nan=True)
        again = eng.svm_kernel(wide[:, :m], gamma, p, out=wide[:, :m])               # in place
        assert np.array_equal(again.cpu().numpy(), want, equal_nan=True), (m, pad, p, "in place")
        assert (wide[:, m:] == -7.0).all()
    fresh = eng.svm_kernel(torch.tensor(D, device="cuda"), 1.0)                      # out=None, p = 1
    assert np.array_equal(fresh.cpu().numpy(), cvr.kernel_matrix(D, 1.0, 1), equal_nan=True)


def test_special_entries(eng):
    D = torch.tensor([[0.0, np.inf, np.nan], [700.1, 50.0, 100.0], [1.0, 2.0, 3.0]], dtype=torch.float32, device="cuda")
    K = eng.svm_kernel(D, 1.0).cpu().numpy()
    assert K[0, 0] == 1.0 and K[0, 1] == 0.0 and np.isnan(K[0, 2]) and K[1, 0] == 0.0
    assert 0 < K[1, 2] < np.finfo(np.float32).tiny                                   # a float32 subnormal survives
    assert abs(float(K[2, 0]) - np.exp(-1.0)) < 1e-7


def test_bad_arguments_are_refused_and_the_context_stays_usable(eng):
    D = torch.rand((8, 8), dtype=torch.float32, device="cuda")
    out = torch.empty((8, 8), dtype=torch.float32, device="cuda")
    L, h, s = eng.L, eng.ctx.handle, eng._stream()
    p = lambda t: t.data_ptr()  # noqa: E731
    bad = [(p(D), 8, 8, 1.0, 0, p(out), 8), (p(D), 8, 8, 0.0, 1, p(out), 8), (p(D), 8, 8, float("inf"), 1, p(out), 8),
           (p(D), 8, 8, float("nan"), 1, p(out), 8), (p(D), 8, 7, 1.0, 1, p(out), 8), (p(D), 8, 8, 1.0, 1, p(out), 7),
           (p(D), 0, 8, 1.0, 1, p(out), 8), (None, 8, 8, 1.0, 1, p(out), 8), (p(D), 8, 8, 1.0, 1, None, 8), (p(D), 8, 8, -1.0, 1, p(out), 8)]
    for a in bad:
        assert L.wdx_svm_kernel_device(h, a[0], a[1], a[2], a[3], a[4], a[5], a[6], s) == _lib.WDX_ERR_INVALID, a
    assert L.wdx_svm_kernel_device(h, p(D), 8, 8, 1.0, _lib.SVM_KERNEL_MAX_POWER + 1, p(out), 8, s) == _lib.WDX_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        eng.svm_kernel(D, -1.0)
    with pytest.raises(ValueError):
        eng.svm_kernel(D.double(), 1.0)
    with pytest.raises(ValueError):
        eng.svm_kernel(D, 1.0, out=torch.empty((7, 8), dtype=torch.float32, device="cuda"))
    got = eng.svm_kernel(D, 0.5, 2)
    assert np.array_equal(got.cpu().numpy(), cvr.kernel_matrix(D.cpu().numpy(), 0.5, 2))


def test_device_entry_enqueues_on_the_callers_stream_without_waiting():
    """the pattern of tests/test_gpu_streams.py: the distances arrive LATE on a side stream; the call returns while the delay is
    still running and gives the serial call's bits"""
    res, _ = so.run_child(HERE, ["stream"], timeout=150.0)
    assert res.get("ok") is True and res["same"] and res["pending"] and res["decoy_differs"], res


def _child_stream():
    _imports()
    A, B, log = so.side_streams()
    print("\n".join(log))
    rng = np.random.default_rng(3)
    real = torch.tensor(rng.gamma(2.0, 2.0, size=(700, 700)).astype(np.float32), device="cuda")
    decoy = torch.tensor(rng.gamma(2.0, 2.0, size=(700, 700)).astype(np.float32), device="cuda")
    e, ref = (DemuxEngine(np.zeros((4, 25)), 15, 0.1) for _ in range(2))
    serial, wrong = ref.svm_kernel(real, 0.3, 2).cpu().numpy(), ref.svm_kernel(decoy, 0.3, 2).cpu().numpy()
    e.svm_kernel(real, 0.3, 2)
    torch.cuda.synchronize()
    t0 = time.time()
    e.svm_kernel(real, 0.3, 2)
    torch.cuda.synchronize()
    ms = so.delay_ms_for(time.time() - t0)
    Dt = torch.empty_like(real)
    ev = so.late(A, [Dt], [real], [decoy], ms)
    with torch.cuda.stream(A):
        res = e.svm_kernel(Dt, 0.3, 2)
        pending = not ev.query()
        got = res.cpu().numpy()
    e.close(), ref.close()
    print(json.dumps(dict(ok=True, same=bool(np.array_equal(got, serial)), pending=pending, decoy_differs=not np.array_equal(wrong, serial), delay_ms=ms)))


if __name__ == "__main__":
    if sys.argv[1:] == ["stream"]:
        _child_stream()
