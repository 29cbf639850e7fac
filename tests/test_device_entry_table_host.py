"""The table of the `_device` entries (tests/helpers/device_entries.py) is closed in both directions, on a machine without a GPU: its
rows are exactly the `_device` names of `_lib.EXPORTS` and exactly the `wdx_\\w+_device(` prototypes of include/wdx.h, so a new entry
without a row -- without exact frames, workspace states and a stream case in tests/test_gpu_device_entries.py -- fails here.  The
sibling table of the `_dev` entries is closed by tests/test_gpu_buffer_bounds.py.

Also here: every argument of every prototype has a role in its row; the kernel constants the cases stand on are the sources' own; the
cases hold the edges they claim (checked on the host, from the rules)."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import device_entries as de  # noqa: E402
from helpers import framed as fr  # noqa: E402
from warpdemux_amd import _lib  # noqa: E402

CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")


def _read(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def _prototypes():
    """name -> the argument names of every `int wdx_..._device(...)` prototype of the header"""
    text = re.sub(r"/\*.*?\*/", " ", _read(ROOT, "include", "wdx.h"), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(wdx_\w+_device)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        out[name] = [re.findall(r"\w+", a)[-1] for a in args.split(",")]
    return out


def test_the_rows_are_the_device_exports_and_the_headers_prototypes():
    rows = set(de.ENTRIES)
    exports = {e for e in _lib.EXPORTS if e.endswith("_device")}
    protos = set(_prototypes())
    assert rows == exports, sorted(rows ^ exports)
    assert rows == protos, sorted(rows ^ protos)
    assert len(rows) == 10


def test_every_array_argument_of_a_prototype_has_a_role_in_its_row():
    scalars = {"ctx", "stream", "n", "L", "n_labels", "window", "penalty", "ld", "ldk", "m", "n_problems", "n_rows", "n_eval", "eps", "max_iter",
               "gamma", "pwr_dist", "n_dec", "k", "n_folds", "resolution", "n_targets"}
    for name, args in _prototypes().items():
        named = {a.name for a in de.ENTRIES[name].args}
        assert set(args) - scalars == named, (name, sorted((set(args) - scalars) ^ named))
        roles = {a.role for a in de.ENTRIES[name].args}
        assert roles <= {de.IN, de.IN_NULLABLE, de.OUT, de.OUT_NULLABLE, de.INOUT, de.HOST, de.HOST_OUT}, (name, roles)


def test_every_row_names_an_engine_method_and_a_rule():
    from warpdemux_amd.engine import DemuxEngine
    from helpers import boost_fit_rule, dba_rule, loo_rule, medoid_rule, self_matrix_rule, svm_cv_rule, svm_fit_rule  # noqa: F401

    without_rule = {"wdx_mlp_fit_device", "wdx_svm_cv_couple_device"}
    for name, e in de.ENTRIES.items():
        assert callable(getattr(DemuxEngine, e.engine)), (name, e.engine)
        if name in without_rule:
            assert "." not in e.rule.split()[0], name
        else:
            mod, fn = e.rule.split(".")
            assert callable(getattr(locals()[mod], fn)), (name, e.rule)


def test_every_case_matches_its_rows_roles():
    """the device arguments of every case are those of its row, by role; the nullable ones are the row's nullable ones; ids are unique"""
    ids = de.case_ids()
    assert len(set(ids)) == len(ids)
    for name, e in de.ENTRIES.items():
        by_role = lambda *r: {a.name for a in e.args if a.role in r}   # noqa: E731
        for c in de.cases(name):
            inplace = set(c.inouts) - by_role(de.INOUT)                # (an input that is also the output: the in-place kernel matrix)
            assert set(c.inputs) | set(c.null_in) | inplace == by_role(de.IN, de.IN_NULLABLE), (name, c.id)
            assert set(c.null_in) <= by_role(de.IN_NULLABLE), (name, c.id)
            assert set(c.outputs) == by_role(de.OUT, de.OUT_NULLABLE) - ({"d_K"} if inplace else set()), (name, c.id)
            assert set(c.nullable) == by_role(de.OUT_NULLABLE), (name, c.id)
            assert set(c.inouts) - inplace == by_role(de.INOUT), (name, c.id)
            for arg, mask in c.written.items():
                size = c.outputs[arg][0] if arg in c.outputs else c.inouts[arg].size
                assert mask.dtype == bool and mask.size == size, (name, c.id, arg)
            for arg, (rows, ld, cols) in c.matrix.items():
                a = c.inputs[arg] if arg in c.inputs else c.inouts[arg]
                assert a.size == (rows - 1) * ld + cols, (name, c.id, arg)       # the payload ends on element (rows-1) ld + cols - 1
                assert ld == cols or np.isnan(a[cols:ld]).all(), (name, c.id, arg)   # NaN in the interior pad columns


def test_the_restated_kernel_constants_are_the_sources_own():
    def const(text, name):
        return int(re.search(r"constexpr \w+ %s\s*=\s*(\d+)" % name, text).group(1))

    assert const(_read(CSRC, "wdx_medoid_plan.h"), "kMedoidChunk") == de.CHUNK_ROWS
    k = _read(CSRC, "wdx_svm_kernel.hip")
    assert const(k, "kSvmKernelPerThread") == de.SVM_KERNEL_VEC
    assert const(k, "kSvmKernelThreads") * const(k, "kSvmKernelPerThread") == de.SVM_KERNEL_COLS
    cv = _read(CSRC, "wdx_svm_cv.hip")
    assert "blockIdx.x * %d + g" % de.CV_ROWS_PER_WAVE in cv and "p += %d" % de.CV_GROUP_LANES in cv
    pairs = lambda k: k * (k - 1) // 2   # noqa: E731
    assert pairs(6) <= de.CV_GROUP_LANES < pairs(7) and 7 in de.CV_CLASSES and max(de.CV_CLASSES) == _lib.SVM_MAX_CLASSES
    t = _read(CSRC, "wdx_thresholds_plan.h")
    assert const(t, "kThrRows") == de.THR_ROWS and const(t, "kThrLdsEntries") == de.THR_LDS_ENTRIES
    assert "top -= %d" % de.THR_SELECT_BINS in _read(CSRC, "wdx_thresholds.hip")
    assert const(_read(CSRC, "wdx_mlp_fit_plan.h"), "kMlpFitRows") == de.MLP_FIT_ROWS
    assert int(re.search(r"#define WDX_BOOST_FIT_ROWS (\d+)", _read(ROOT, "include", "wdx.h")).group(1)) == de.BOOST_FIT_ROWS
    assert (_lib.OPT_DBA_GENERAL, _lib.OPT_SELF_NEAREST_GENERAL) == (de.OPT_DBA_GENERAL, de.OPT_SELF_NEAREST_GENERAL)
    assert fr.GUARD >= 64 * 1024


def test_the_solver_case_holds_all_three_states_and_the_thresholds_cases_a_second_class_group():
    c = de.case("wdx_svm_solve_device", "m40-ld41")
    want = c.rule()
    states = set(int(s) for s in want["d_state"])
    assert states == {0, 1, 2}, states
    K, batch, _ = de.svm_solve_batch()
    assert len(batch.problems) > 3 and (batch.problems["n_eval"] > 0).any() and (batch.kind == -1).sum() == 3
    # a stopped problem's alpha stays in its slice: the rule's own alpha of the other problems is what the device must return
    assert c.outputs["d_alpha"][0] == len(batch.rows) and c.outputs["d_dec"][0] == len(batch.eval_rows)
    groups = []
    for t in de.cases("wdx_accuracy_thresholds_device"):
        n, k, R, T = (int(v) for v in re.match(r"n(\d+)-k(\d+)-R(\d+)-T(\d+)", t.id).groups())
        fit = de.THR_LDS_ENTRIES // (2 * (R + 1))
        groups.append(-(-k // min(fit, k)))
    assert max(groups) >= 2 and min(groups) == 1


def test_every_row_has_a_late_input_case_here_or_in_its_own_file():
    """the four of tests/test_gpu_device_entries.py and the six whose own files hold them to it: a new row has to be put into one of
    the two lists, and a listed file has to name its entry in a stream child"""
    assert set(de.LATE_HERE) | set(de.LATE_ELSEWHERE) == set(de.ENTRIES) and not set(de.LATE_HERE) & set(de.LATE_ELSEWHERE)
    for name, (cid, _) in de.LATE_HERE.items():
        assert de.case(name, cid) is not None
    for name, path in de.LATE_ELSEWHERE.items():
        text = _read(ROOT, "tests", path)
        assert "def _child_stream" in text and ("." + name + "(" in text or de.ENTRIES[name].engine + "(" in text), (name, path)
    a, b = (re.match(r"n\d+-k(\d+)-R(\d+)", cid).groups() for cid in de.THR_WS_PAIR)
    assert a[0] != b[0] and a[1] != b[1], "the two calls of the thr_ws stream case differ in k and in R"


def test_the_dba_cases_take_the_routes_they_name():
    """wdx_dba_plan.h: dba_kernel -- the general route when the option is set or the effective window exceeds kMaxRegWindow"""
    plan = _read(CSRC, "wdx_dba_plan.h")
    assert "if (opt_general || w > kMaxRegWindow) return DbaKernel::kGeneral;" in plan
    assert int(re.search(r"constexpr int kMaxRegWindow = (\d+);", _read(CSRC, "wdx_dtw_plan.h")).group(1)) == de.DTW_MAX_REG_WINDOW
    general = lambda c, L, w: dict(c.options)[de.OPT_DBA_GENERAL] == 1 or (L if w <= 0 or w > L else w) > de.DTW_MAX_REG_WINDOW   # noqa: E731
    band, gen = de.case("wdx_dba_step_device", "window15-band"), de.case("wdx_dba_step_device", "window0-general")
    assert not general(band, de.L_DTW, de.WINDOW) and not general(band.big(), 31, 9)
    assert general(gen, de.L_DTW, 0) and general(gen.big(), 31, 0)
    assert len(de.cases("wdx_dba_step_device")) == 2


def test_the_coupling_reference_holds_rows_in_every_case():
    """the probability bound of a wdx_svm_cv_couple_device case applies beyond the reference's stopping margin: in every case that is
    most of the finite rows, never none"""
    for c in de.cases("wdx_svm_cv_couple_device"):
        assert c.finite_rows >= 1 and c.reference_rows() >= max(1, c.finite_rows - 1), (c.id, c.reference_rows(), c.finite_rows)


def test_only_the_coupling_row_answers_through_ctypes_on_the_second_context():
    assert {n for n, e in de.ENTRIES.items() if e.second != "method"} == {"wdx_svm_cv_couple_device"}
    assert {e.second for e in de.ENTRIES.values()} == {"method", "ctypes"}
