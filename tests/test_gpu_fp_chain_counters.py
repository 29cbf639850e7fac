"""Which list each launch of the fingerprint chain takes and feeds: what the replay of the route table
(tests/test_fp_plan_host.py) cannot see.  Nine cases of 4 096 reads with WDX_OPT_FAST_CHAIN_MIN_READS = 1024 -- W12 / d6 with
the windows cut to 4096, 5120, 6144, 8192, 12288 and 16384 samples, W30 / d15, refinement at W18 / d9 (every 64th read with a
barcode tail beyond the tail kernel, as tests/test_gpu_buffer_bounds.py builds them), W13 -- through the public engine; after
each call the eight counters at the front of the fingerprint piece of d_work (tests/helpers/framed.py says where) and the
launches the call reports must be those of tests/golden/fp_chain_counters.json, which tools/record_chain_counters.py wrote on
the tree BEFORE the launch code became a plan and a step runner.  A launch that took, handed over to or retried on another list
than before, or from another entry, leaves other counts.  The recording itself is acceptable only if every list held reads
somewhere: slow, big0, big1, retry and big2 in some case, back in the refinement case.

The file keeps, per counter, the lowest and highest value over the recordings (24 plain and 60 with other work beside the
calls, merged).  They agree everywhere but for slow and retry in cases whose big0 list is longer than the 1 024-workgroup grid of
its one-workgroup-per-entry kernel: there the order of the list's entries -- which workgroup won the atomic first -- decides
which of two kernels a read takes (the script says more), and the tree before the plan itself gives retry 1 026 .. 1 027 (5 120),
slow 10 .. 14 and retry 9 .. 13 (6 144), retry 4 .. 6 (8 192).  Only there may a value lie in the recorded range widened by
itself once; everywhere else it must be the recorded one."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_chain_counters", os.path.join(ROOT, "tools", "record_chain_counters.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(rec.GOLDEN) as _fh:
    GOLDEN = json.load(_fh)


def test_the_recording_used_every_list():
    assert sorted(GOLDEN) == sorted(rec.CASES) and len(GOLDEN) == 9
    assert rec.acceptable(GOLDEN) == []
    assert all(set(r) == set(rec.fr.COUNTER_NAMES) | {"n_launches", "n_launches_main"} for r in GOLDEN.values())


@pytest.mark.parametrize("name", list(rec.CASES))
def test_counters_and_launches_are_the_recorded_ones(name):
    got = rec.record(name)
    print(name, got)
    assert set(got) == set(GOLDEN[name])
    for counter, lo_hi in GOLDEN[name].items():
        assert lo_hi[0] == lo_hi[1] or (counter in ("slow", "retry") and GOLDEN[name]["big0"][0] > rec.GRID), (name, counter, lo_hi)
        assert got[counter] in rec.allowed(lo_hi), (name, counter, got[counter], lo_hi)
