"""The int16 device shards without a GPU: the slicing arithmetic of warpdemux_amd/csrc/wdx_adc_dev.h -- pitch, reads per
slice, staging bytes, number of slices -- and the window the device kernel stages for a read.  tests/host/adc_dev_check.cpp
is built with the system C++ compiler under the address and undefined-behaviour sanitizers; its answers are compared with
the arithmetic as the issue states it, written out here independently, and the program itself asserts that the staged window
is `adapter_window`'s (wdx_window.h) and stays inside the pitch and inside the read.  A second test checks the ABI layer."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

from warpdemux_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "adc_dev_check.cpp")
BUDGET = 1 << 30                      # the stated staging budget
MAX_LENS = (1, 255, 6144, 16384, 65536)


def _pitch(max_len):
    return (max_len + 8 + 7) // 8 * 8   # round_up(max_len + 8, 8)


def _builtin_slice(max_len):
    return BUDGET // (_pitch(max_len) * 4 + 12)


def _plan_cases():
    rows = []
    for max_len in MAX_LENS:
        built_in = _builtin_slice(max_len)
        for opt in (0, 1, 100, built_in - 1, built_in, built_in + 1, 1 << 40):
            sl = min(opt, built_in) if opt > 0 else built_in
            for n in (0, 1, sl - 1, sl, sl + 1, 1 << 31):
                rows.append([0, n, max_len, opt, 0, 0, 0, 0, 0])
    return np.array(rows, dtype=np.int64)


def _plan_rule(c):
    out = []
    for _, n, max_len, opt, *_ in c.tolist():
        pitch = _pitch(max_len)
        sl = _builtin_slice(max_len)
        if opt > 0:
            sl = min(sl, opt)           # the option overrides the built-in, inside the budget
        n_slices = -(-n // sl)
        last = n - (n_slices - 1) * sl if n else 0
        out.append([pitch, sl, n_slices, last, min(n, sl) * (pitch * 4 + 12), BUDGET])
    return np.array(out, dtype=np.int64)


def _window_cases():
    """kind 1 records: a_start a_end packed|2*dead capacity row_len row_win padding max_len"""
    rows = []
    # a small row, every start (so every residue mod 8), every end, inverted and empty windows, starts beyond the row, windows
    # past row_len (NaN tail) and past the cut, dead reads -- strided and packed, with and without row_win
    pos = np.arange(-3, 45)
    for packed, cap, row_len, row_win in ((0, 32, 20, -1), (0, 32, 40, -1), (0, 29, -2, -1), (1, 24, 20, -1), (1, 24, 20, 30),
                                          (1, 24, 20, 7), (1, 8, 30, 12), (1, 0, 0, 0)):
        for dead in (0, 1):
            for padding in (0, 1, 5):
                for max_len in (1, 9, 64):
                    g = np.stack(np.meshgrid(pos, pos, indexing="ij"), axis=-1).reshape(-1, 2)
                    k = np.tile(np.array([[1, 0, 0, packed | (dead << 1), cap, row_len, row_win, padding, max_len]]), (len(g), 1))
                    k[:, 1:3] = g
                    rows.append(k)
    # the production shapes: the five max_len values, windows at, one short of and one beyond them
    for max_len in MAX_LENS:
        for start in range(100, 108):
            for extra in (-1, 0, 1, 2, 9):
                rows.append(np.array([[1, start + 100, start + 100 + max_len - 200 + extra, 0, 70000, 69000, -1, 100, max_len]]))
    rows.append(np.array([[1, 2_000_000, 2_000_500, 2, 9000, 8000, -1, 100, 6144],      # garbage start of a dead read
                          [1, 9500, 9900, 0, 9000, 8000, -1, 100, 6144],                 # a start beyond the row
                          [1, 3000, 8950, 0, 9000, 8000, -1, 100, 6144]]))               # a window past row_len
    return np.concatenate(rows).astype(np.int64)


def _window_rule(c):
    """extract_adapter's window on the float32 row the read stands for, cut one sample beyond max_len, packed from the last
    multiple of 8 at or before its first sample; `valid` counted against the read's own (clamped) samples"""
    _, a_s, a_e, flags, cap, row_len, row_win, pad, max_len = c.T
    packed, dead = flags & 1, flags >> 1
    cap = np.maximum(cap, 0)
    rl = np.clip(row_len, 0, cap)
    limit = np.where(packed == 1, np.maximum(row_win, rl), cap)
    st = np.minimum(np.maximum(a_s - pad, 0), limit)
    en = np.minimum(np.minimum(a_e + pad, limit), st + max_len + 1)
    live = (dead == 0) & (en > st)
    first = np.where(live, st - st % 8, 0)
    row = np.where(live, en - first, 0)
    valid = np.clip(rl - first, 0, row)
    win = np.where(live, en - st, 0)
    return np.stack([first, row, valid, win, a_s - first, a_e - first], axis=1)


def _build(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "adc_dev_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe])
    return exe


def _run(exe, cases):
    run = subprocess.run([exe], input=np.ascontiguousarray(cases, dtype="<i8").tobytes(), capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr.decode().strip().endswith("%d cases" % cases.shape[0]), run.stderr[-2000:]
    return np.frombuffer(run.stdout, dtype="<i8").reshape(-1, 6)


def test_slicing_arithmetic_and_staged_windows_under_sanitizers(tmp_path):
    exe = _build(tmp_path)
    plans = _plan_cases()
    got, want = _run(exe, plans), _plan_rule(plans)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (plans[bad[0]], got[bad[0]], want[bad[0]])
    assert (got[:, 4] <= BUDGET).all(), "staging never above the stated budget"
    assert (got[plans[:, 1] == 1 << 31, 2] > 1).all(), "2^31 reads are walked in slices, without overflow"
    # the pitch of the longest window still leaves thousands of reads per slice
    assert _builtin_slice(65536) >= 4000 and _pitch(65536) == 65544

    wins = _window_cases()
    assert wins.shape[0] > 300_000
    got, want = _run(exe, wins), _window_rule(wins)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (wins[bad[0]], got[bad[0]], want[bad[0]])
    assert len(set((got[got[:, 1] > 0, 4] % 8).tolist())) == 8, "starts at every residue mod 8"
    assert (got[:, 3] > wins[:, 8]).any(), "windows beyond max_len are staged one sample too long: the chain reports them"


def test_adc_dev_abi_is_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "wdx.h")).read()
    twins = ["wdx_fingerprint_adc_dev", "wdx_fingerprint_refine_adc_dev", "wdx_demux_adc_dev", "wdx_demux_refine_adc_dev",
             "wdx_demux_svm_adc_dev", "wdx_demux_mlp_adc_dev", "wdx_demux_boost_adc_dev"]
    sizes = ["wdx_demux_adc_workspace_bytes", "wdx_demux_refine_adc_workspace_bytes", "wdx_adc_dev_staging_bytes"]
    L = _lib.load()
    for name in twins + sizes:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
        # one ctypes argument per parameter of the declaration
        decl = re.search(r"^int(?:64_t)? %s\(([^;]*)\);" % name, hdr, flags=re.M).group(1)
        assert len(getattr(L, name).argtypes) == decl.count(",") + 1, name
        # ... and the twin takes the float32 entry's parameters with the shard in place of sig / row_off / row_len / stride
        if name in twins:
            f32 = re.search(r"^int %s\(([^;]*)\);" % name.replace("_adc_dev", "_dev"), hdr, flags=re.M).group(1)
            assert decl.count(",") == f32.count(",") - 3, name
    assert re.search(r"^#define\s+WDX_OPT_ADC_DEV_SLICE_READS\s+(\d+)", hdr, flags=re.M).group(1) == str(_lib.OPT_ADC_DEV_SLICE_READS)
    assert re.search(r"^#define\s+WDX_K_ADC_DEV_WINDOWS\s+(\d+)", hdr, flags=re.M).group(1) == str(_lib.K_ADC_DEV_WINDOWS)
    body = hdr[hdr.index("typedef struct wdx_adc_dev_in {"): hdr.index("} wdx_adc_dev_in;")]
    fields = re.findall(r"\*?(\w+)(?:,\s*\*(\w+))?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    names = [n for pair in fields for n in pair if n]
    assert names == [f[0] for f in _lib.AdcDevInC._fields_], names
    assert ctypes.sizeof(_lib.AdcDevInC) == 56
    assert L.wdx_abi_version() == 4
    # the size functions refuse a null context with 0 instead of reading through it
    assert L.wdx_demux_adc_workspace_bytes(None, 10, 100, 25) == 0 and L.wdx_adc_dev_staging_bytes(None, 10, 100, 0) == 0


def test_every_device_buffer_of_the_context_is_released_with_it():
    """wdx_ctx_destroy frees the context's device blocks through an explicit list and `wdx::Buffer` has no destructor: a
    buffer that is declared in the context and missing from that list -- the int16 shards' staging block, up to 1 GiB -- leaks
    with every context that used it"""
    ctx_h = open(os.path.join(CSRC, "wdx_ctx.h")).read()
    body = ctx_h[ctx_h.index("struct wdx_ctx {"): ctx_h.index("namespace wdx {\n\nstruct Timed")]
    body = re.sub(r"//[^\n]*", "", body)
    declared = [n.strip() for m in re.finditer(r"wdx::Buffer\s+([^;]+);", body) for n in m.group(1).split(",")]
    assert "adc_stage" in declared and "fp_ws" in declared and len(declared) > 30, declared
    api = open(os.path.join(CSRC, "wdx_api.hip")).read()
    destroy = api[api.index("void wdx_ctx_destroy(wdx_ctx *ctx) {"): api.index("int wdx_ctx_set_option(")]
    released = set(re.findall(r"&ctx->(\w+)", destroy))
    assert not [n for n in declared if n not in released], [n for n in declared if n not in released]
    # ... and the staging block is allocated without the head-room of the other workspaces: its size is a stated bound
    assert re.search(r"adc_stage\.ensure\(\(size_t\)plan\.staging_bytes, true\)", ctx_h)
