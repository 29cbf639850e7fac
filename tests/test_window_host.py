"""The adapter-window rule of every host way in (warpdemux_amd/csrc/wdx_window.h), exhaustively over its small domain and
without a GPU: tests/host/window_check.cpp is built with the system C++ compiler under the address and undefined-behaviour
sanitizers, run on every case, and its answers are compared with the rule as stated here from extract_adapter
(sig_proc.py:382-391).  The program itself asserts the bounds and the "same window" claim of every case."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "window_check.cpp")
NO_LIMIT = np.iinfo(np.int64).max


def _grid(*axes):
    return np.stack([g.ravel() for g in np.meshgrid(*[np.asarray(a, np.int64) for a in axes], indexing="ij")], axis=1)


def _cases():
    """columns: a_start a_end limit padding align max_win row_len dead (limit -1: none; row_len -1: no valid count)"""
    blocks = []
    for limit in (0, 1, 7, 8, 9, 16):
        pos = np.arange(-3, limit + 13)
        blocks.append(_grid(pos, pos, [limit], [0, 1, 5], [1, 4, 8], [0], np.arange(-1, limit + 1), [0, 1]))
    # the live tick's int16 windows: no row limit, the cap shrunk to 3 samples
    pos = np.arange(-3, 29)
    blocks.append(_grid(pos, pos, [-1], [0, 1, 5], [1, 4, 8], [3], np.arange(-1, 17), [0, 1]))
    return np.concatenate(blocks)


def _rule(c):
    """extract_adapter's window [max(0, a_start - padding), min(limit, a_end + padding)), its start clamped to the row, at most
    max_win samples of it; packed from the last multiple of `align` at or before its first sample"""
    a_s, a_e, limit, pad, align, cap, row_len, dead = c.T
    lim = np.where(limit < 0, NO_LIMIT, limit)
    st = np.minimum(np.maximum(a_s - pad, 0), lim)
    en = np.minimum(a_e + pad, lim)
    en = np.where(cap > 0, np.minimum(en, st + cap), en)
    live = (dead == 0) & (en > st)
    first = np.where(live, st - st % align, 0)
    row = np.where(live, en - first, 0)
    valid = np.where(row_len < 0, row, np.clip(row_len - first, 0, row))
    win = np.where(live, en - st, 0)
    return np.stack([first, row, valid, win, a_s - first, a_e - first], axis=1)


def test_window_rule_exhaustively_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "window_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe])
    cases = _cases()
    assert cases.shape[0] > 300_000
    run = subprocess.run([exe], input=np.ascontiguousarray(cases, dtype="<i8").tobytes(), capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr.decode().strip().endswith("%d cases" % cases.shape[0]), run.stderr[-2000:]
    got = np.frombuffer(run.stdout, dtype="<i8").reshape(-1, 6)
    want = _rule(cases)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (cases[bad[0]], got[bad[0]], want[bad[0]])
    # the properties again, on the answers: nothing outside the row, aligned, valid within the packed row
    first, row, valid = got[:, 0], got[:, 1], got[:, 2]
    lim = np.where(cases[:, 2] < 0, NO_LIMIT, cases[:, 2])
    assert (first >= 0).all() and (first <= lim).all() and (first + valid <= lim).all()
    assert (first % cases[:, 4] == 0).all() and (valid <= row).all() and (valid >= 0).all()
    # the edge the float32 ways in used to get wrong: a start at or beyond the row takes nothing
    beyond = (cases[:, 0] - cases[:, 3] >= cases[:, 2]) & (cases[:, 2] >= 0)
    assert beyond.any() and (row[beyond] == 0).all() and (valid[beyond] == 0).all()
