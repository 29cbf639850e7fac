"""wdx_live_tick_ex and the Python live layer over it, as far as they can be checked without a GPU: the export and its
ctypes signature, the header's WDX_LIVE_TAIL_* values and the layout of wdx_live_in against `_lib.LiveInC` (parsed from
include/wdx.h in the style of tests/test_boost_paths_host.py), and every refusal of `LiveDemux(...)` / `demux_worker` that
is raised before a context exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import boost_ref
from warpdemux_amd import _lib, live, models, sig_proc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 25


def _hdr():
    return open(os.path.join(ROOT, "include", "wdx.h")).read()


def _boost(n_features=K, dim=4):
    m = boost_ref.random_model(3, 2, dim, n_features, seed=1)
    trees = [(f, b, [False] * len(f), lv) for f, b, lv in m.trees]
    return models.Fpt_Boost(trees, m.n_features, m.scale, m.bias, {i: i for i in range(m.k)})


def _svm(L=K, n_train=6, k=3):
    """a DTW_SVM's host side only (nothing is fitted: the constructor checks read shapes)"""
    n_sv = n_train
    return models.DTW_SVM(np.zeros((n_train, L)), [2] * k, np.arange(n_sv), np.zeros((k - 1, n_sv)), np.zeros(k * (k - 1) // 2),
                          np.zeros(k * (k - 1) // 2), np.zeros(k * (k - 1) // 2), {i: i for i in range(k)}, None, 15, 0.1)


def _mlp(L=K, nY=6, k=3):
    return models.DTW_MLP(np.zeros((nY, L)), [np.zeros((nY, 4), np.float32), np.zeros((4, k), np.float32)],
                          [np.zeros(4, np.float32), np.zeros(k, np.float32)], "relu", {i: i for i in range(k)}, None, 15, 0.1)


def _refine(keep=K):
    return sig_proc.RefineParams(query=np.linspace(-1.0, 1.0, 84), barcode_keep_events=keep)


def test_the_library_exports_the_tick_and_the_binding_names_it():
    L = _lib.load()
    assert "wdx_live_tick_ex" in _lib.EXPORTS
    f = L.wdx_live_tick_ex
    P = C.POINTER
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_void_p, P(_lib.LiveInC), P(_lib.SegParamsC), P(_lib.RefineParamsC), C.c_int64, C.c_uint32,
                          P(_lib.MinibatchOutC), C.c_void_p, P(C.c_int64)]
    # ... and the header declares it with that argument list
    decl = re.search(r"int wdx_live_tick_ex\(([^;]*)\);", _hdr()).group(1)
    assert [re.sub(r"\s*\*", "*", re.sub(r"\w+$", "", " ".join(a.split())).strip()) for a in decl.split(",")] == [
        "wdx_ctx*", "const wdx_live_in*", "const wdx_seg_params*", "const wdx_refine_params*", "int64_t", "uint32_t",
        "const wdx_minibatch_out*", "int32_t*", "int64_t*"]
    assert L.wdx_abi_version() == 4 == _lib.ABI_VERSION     # additive: the version stays


def test_tail_values_and_the_structure_layout_mirror_the_header():
    hdr = _hdr()

    def define(name):
        return int(re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", hdr, flags=re.M).group(1), 0)

    assert (_lib.LIVE_TAIL_NONE, _lib.LIVE_TAIL_SVM, _lib.LIVE_TAIL_MLP, _lib.LIVE_TAIL_BOOST) == tuple(
        define("WDX_LIVE_TAIL_" + t) for t in ("NONE", "SVM", "MLP", "BOOST")) == (0, 1, 2, 3)
    # wdx_live_in, field by field: name, size and alignment from the C declaration (LP64), offsets by the C rule
    body = re.search(r"typedef struct wdx_live_in \{(.*?)\} wdx_live_in;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        first, *more = [d.strip() for d in stmt.split(",")]
        base, name = first.rsplit(" ", 1)
        for nm in [name] + more:
            pointer = nm.startswith("*") or base.endswith("*")
            size = 8 if pointer else {"int64_t": 8, "int32_t": 4, "uint32_t": 4}[base.replace("const ", "")]
            fields.append((nm.lstrip("*"), size))
    off, expect = 0, []
    for name, size in fields:
        off = (off + size - 1) // size * size
        expect.append((name, off, size))
        off += size
    total = (off + 7) // 8 * 8
    got = [(n, getattr(_lib.LiveInC, n).offset, getattr(_lib.LiveInC, n).size) for n, _ in _lib.LiveInC._fields_]
    assert got == expect
    assert [n for n, _, _ in expect] == ["rows", "adc_rows", "offset", "scale", "row_len", "n_reads", "a_start", "a_end", "ok",
                                         "tail", "pad_"]
    assert C.sizeof(_lib.LiveInC) == total == 80


def test_constructor_refusals_come_before_a_context():
    made = []
    orig = _lib.Context
    _lib.Context = lambda *a, **k: made.append(1) or (_ for _ in ()).throw(AssertionError("a context was created"))
    try:
        # model kind
        with pytest.raises(ValueError, match="DTW_SVM, DTW_MLP and Fpt_Boost"):
            live.LiveDemux(np.zeros((3, K)), 15, 0.1, model=object())
        # K against the reference length / n_features / barcode_keep_events
        with pytest.raises(ValueError, match=r"barcode_num_events \(24\) must equal the reference length \(25\)"):
            live.LiveDemux(np.zeros((3, K)), 15, 0.1, sig_proc.SegParams(barcode_num_events=24))
        with pytest.raises(ValueError, match="reference length"):
            live.LiveDemux(params=sig_proc.SegParams(barcode_num_events=24), model=_svm())
        with pytest.raises(ValueError, match="reference length"):
            live.LiveDemux(params=sig_proc.SegParams(barcode_num_events=24), model=_mlp())
        with pytest.raises(ValueError, match=r"n_features \(25\)"):
            live.LiveDemux(params=sig_proc.SegParams(barcode_num_events=24), model=_boost())
        with pytest.raises(ValueError, match=r"barcode_keep_events \(20\) must equal the boost model's n_features"):
            live.LiveDemux(model=_boost(), refine=_refine(20))
        with pytest.raises(ValueError, match=r"barcode_keep_events \(20\) must equal the reference length"):
            live.LiveDemux(np.zeros((3, K)), 15, 0.1, refine=_refine(20))
        with pytest.raises(ValueError, match="must equal the boost model's n_features"):
            live.LiveDemux(np.zeros((3, 24)), 15, 0.1, model=_boost())
        with pytest.raises(ValueError, match="reference length"):
            live.LiveDemux(np.zeros((3, 24)), 15, 0.1, sig_proc.SegParams(barcode_num_events=K), model=_boost())
        # refinement with a DTW model
        with pytest.raises(ValueError, match="consensus refinement .* DTW_SVM"):
            live.LiveDemux(model=_svm(), refine=_refine())
        with pytest.raises(ValueError, match="consensus refinement .* DTW_MLP"):
            live.LiveDemux(model=_mlp(), refine=_refine())
        with pytest.raises(ValueError, match="consensus query"):
            live.LiveDemux(model=_boost(), refine=sig_proc.RefineParams(query=None))
        # no references and nothing that could do without them
        with pytest.raises(ValueError, match="refs may only be None with an Fpt_Boost"):
            live.LiveDemux(None)
        with pytest.raises(ValueError, match="refs may only be None with an Fpt_Boost"):
            live.LiveDemux(None, refine=_refine())
        with pytest.raises(ValueError, match=r"refs must be \(nY, K\)"):
            live.LiveDemux(np.zeros(K), 15, 0.1)
    finally:
        _lib.Context = orig
    assert not made


def test_demux_worker_still_refuses_a_live_demux_without_a_model():
    ld = live.LiveDemux.__new__(live.LiveDemux)    # the refusal is the worker's first statement: the field alone
    ld.k = 0
    with pytest.raises(ValueError, match="needs a LiveDemux with a"):
        live.demux_worker(None, None, ld)
