"""The accuracy-threshold rule restated in NumPy (warpdemux_amd/_thresholds.py: rule; include/wdx.h states it) against a brute
force that sorts and counts (tests/helpers/svm_cv_rule.py), the target conversion, and the reference's threshold table read and
written back byte for byte.  No device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import svm_cv_rule as cvr  # noqa: E402
from warpdemux_amd import _thresholds, file_formats  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "target_accuracy_thresholds_WDX4_rna004.csv")


def _random_case(n, k, seed, noise=0.3):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, k, n).astype(np.int32)
    logits = rng.normal(size=(n, k)) + 3.0 * (np.arange(k)[None, :] == y[:, None])
    swap = rng.random(n) < noise
    y[swap] = rng.integers(0, k, int(swap.sum()))
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True), y


def _same(got, want):
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert int(got[3]) == int(want[3])


@pytest.mark.parametrize("n,k,R", [(1, 2, 1), (200, 2, 10), (500, 4, 100), (300, 10, 37), (400, 16, 100)])
def test_rule_equals_the_sort_based_brute_force(n, k, R):
    prob, y = _random_case(n, k, seed=n + k)
    prob[::17] = np.round(prob[::17], 2)          # margins that sit on or next to grid values
    if n > 20:
        y[3] = -1
        prob[5, 1] = np.nan
        prob[7, 0] = np.inf
    pm = np.array([0, 500, 950, 990, 999, 1000], np.int32)
    _same(_thresholds.rule(prob, y, pm, R), cvr.thresholds_brute(prob, y, pm, R))


def test_thresholds_do_not_decrease_as_the_target_rises():
    prob, y = _random_case(3000, 6, seed=2)
    pm = np.array([0, 800, 900, 950, 990, 999, 1000], np.int32)
    thr = _thresholds.rule(prob, y, pm, 100)[0]
    assert (thr[1:] >= thr[:-1]).all()
    assert np.isfinite(thr[0]).all() and (thr[0] >= 0.01).all()      # target 0: the lowest bin that holds a row, never below 1 / R


def test_infinite_for_a_class_never_predicted_and_for_an_unreachable_target():
    prob = np.array([[0.7, 0.2, 0.1], [0.6, 0.3, 0.1], [0.1, 0.8, 0.1], [0.2, 0.7, 0.1]])
    y = np.array([0, 0, 1, 0], np.int32)          # class 1 is right once in two calls; class 2 is never called
    thr, kept, hit, skipped = _thresholds.rule(prob, y, np.array([500, 1000], np.int32), 100)
    assert skipped == 0 and np.isinf(thr[:, 2]).all() and kept[2].sum() == 0
    assert np.array_equal(thr[:, 0], [0.01, 0.01])
    # class 1: the row with margin 0.8 - 0.1 is right, the one with 0.7 - 0.2 (just below 0.5: bin 49) is not ...
    assert thr[0, 1] == 0.01 and thr[1, 1] == np.float64(50) / np.float64(100)
    y[2] = 0
    assert np.isinf(_thresholds.rule(prob, y, np.array([1000], np.int32), 100)[0][0, 1])   # ... and with neither right: never


def test_a_margin_on_a_grid_value_is_kept_at_that_value():
    R = 100
    for i in (1, 7, 29, 58, 99, 100):
        g = np.float64(i) / np.float64(R)
        for conf, bin_ in ((g, i), (np.nextafter(g, 0.0), i - 1), (np.nextafter(g, 2.0), i)):
            prob = np.array([[conf, 0.0]])         # top1 - top2 = conf exactly
            thr, kept, hit, _ = _thresholds.rule(prob, np.array([0], np.int32), np.array([1000], np.int32), R)
            assert kept[0, bin_] == 1 and (bin_ == R or kept[0, bin_ + 1] == 0), (i, conf)
            assert thr[0, 0] == 0.01 if bin_ >= 1 else np.isinf(thr[0, 0])


def test_targets_are_whole_numbers_of_per_mille():
    assert _thresholds.targets_per_mille((0.95, 0.995, 0.999, 0.0, 1.0)).tolist() == [950, 995, 999, 0, 1000]
    assert _thresholds.targets_per_mille(0.99).tolist() == [990]
    for bad in (0.9995, 1.2, -0.1, float("nan"), ()):
        with pytest.raises(ValueError):
            _thresholds.targets_per_mille(bad)
    with pytest.raises(ValueError):
        _thresholds.rule(np.zeros((3, 1)), np.zeros(3, np.int32), [990], 100)
    with pytest.raises(ValueError):
        _thresholds.rule(np.zeros((3, 2)), np.zeros(3, np.int32), [990], 5000)


def test_reference_threshold_table_round_trips_byte_for_byte(tmp_path):
    mapper, table, targets = file_formats.read_accuracy_thresholds(FIXTURE)
    assert mapper == {0: 3, 1: 4, 2: 5, 3: 7} and targets == [0.95, 0.96, 0.97, 0.98, 0.99, 0.995, 0.999]
    assert table.shape == (7, 4) and table[4].tolist() == [0.17, 0.28, 0.23, 0.47]
    out = tmp_path / "thr.csv"
    file_formats.write_accuracy_thresholds(str(out), mapper, table, targets)
    assert out.read_bytes() == open(FIXTURE, "rb").read()
    table[6, 2] = np.inf                            # "call nothing of this class" survives the file
    file_formats.write_accuracy_thresholds(str(out), mapper, table, targets)
    assert np.array_equal(file_formats.read_accuracy_thresholds(str(out))[1], table)
    with pytest.raises(ValueError):
        file_formats.write_accuracy_thresholds(str(out), mapper, table[:3], targets)
