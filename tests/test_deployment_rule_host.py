"""What a `MinibatchPipeline`, a `Feeder` and a `LiveDemux` serve is ONE rule (`_marshal.deployment`): one table of argument
combinations, each run against all three constructors.  Where a class accepts the combination, the resolved (nY, K) or the
refusal is the same in all of them; where a class does not serve it -- its own statement: a `MinibatchPipeline` takes an
`Fpt_Boost` only, a `Feeder` no `DTW_MLP`, a `LiveDemux` no refinement without a model or references and none in front of a
DTW model -- it says so.  No row gets as far as the library: every refusal is a ValueError before a context, a ring or a
process exists."""
import numpy as np
import pytest

from test_live_ex_host import _boost, _mlp, _refine, _svm
from warpdemux_amd import _lib, feeder, live, pipeline, sig_proc

K = 25
CLASSES = {"pipeline": pipeline.MinibatchPipeline, "feeder": feeder.Feeder, "live": live.LiveDemux}
NOTHING = {"pipeline": "refs is required", "feeder": "refs or model is required", "live": "refs may only be None with an Fpt_Boost"}


def _p(k):
    return sig_proc.SegParams(barcode_num_events=k)


def _refs(k=K, n=3):
    return np.zeros((n, k))


# (name, constructor arguments, the answer of every class that accepts the combination: (nY, K) or the refusal's text,
#  {class: its own refusal} for the classes that do not serve the combination)
ROWS = [
    ("refs", dict(refs=_refs()), (3, K), {}),
    ("refs, window and penalty, K from params", dict(refs=_refs(), window=15, penalty=0.1, params=_p(K)), (3, K), {}),
    ("params against the reference length", dict(refs=_refs(), params=_p(24)),
     r"barcode_num_events \(24\) must equal the reference length \(25\)", {}),
    ("keep events against the reference length", dict(refs=_refs(24), refine=_refine(25)),
     r"barcode_keep_events \(25\) must equal the reference length \(24\)", {}),
    ("keep events against the reference length, the other way", dict(refs=_refs(), refine=_refine(20)),
     r"barcode_keep_events \(20\) must equal the reference length \(25\)", {}),
    ("refinement in front of references", dict(refs=_refs(), refine=_refine(), params=_p(7)), (3, K), {}),
    ("nothing to serve", dict(), None, NOTHING),
    ("nothing to serve, spelled out", dict(refs=None, refine=None, model=None), None, NOTHING),
    ("refinement alone: fingerprints only", dict(refine=_refine()), (0, K), {"live": NOTHING["live"]}),
    ("refinement alone, K = keep events", dict(refine=_refine(20), params=_p(K)), (0, 20), {"live": NOTHING["live"]}),
    ("1-D refs", dict(refs=np.zeros(K)), r"refs must be \(nY, K\)", {}),
    ("refinement without a query", dict(refs=_refs(), refine=sig_proc.RefineParams(query=None)), "consensus query", {}),
    ("not a model", dict(refs=_refs(), model=object()), None,
     {"pipeline": "MinibatchPipeline serves models.Fpt_Boost, not object", "feeder": "Feeder serves models.DTW_SVM and Fpt_Boost, not object",
      "live": "LiveDemux serves models.DTW_SVM, DTW_MLP and Fpt_Boost, not object"}),
    ("boost model alone", dict(model=_boost()), (0, K), {}),
    ("boost model behind refinement", dict(model=_boost(), refine=_refine()), (0, K), {}),
    ("boost model beside references", dict(refs=_refs(), model=_boost(), refine=_refine()), (3, K), {}),
    ("params against the boost model", dict(model=_boost(), params=_p(24)),
     r"boost model takes 25 features: barcode_num_events \(24\) must equal the boost model's n_features \(25\)", {}),
    ("keep events against the boost model", dict(model=_boost(), refine=_refine(20)),
     r"boost model takes 25 features: refine.barcode_keep_events \(20\) must equal the boost model's n_features \(25\)", {}),
    ("reference length against the boost model", dict(refs=_refs(24), model=_boost()),
     r"barcode_num_events \(24\) must equal the boost model's n_features \(25\)", {}),
    ("the reference length is checked before the boost model", dict(refs=_refs(24), params=_p(K), model=_boost()),
     r"barcode_num_events \(25\) must equal the reference length \(24\)", {}),
    ("DTW_SVM: its _X are the references", dict(model=_svm()), (6, K), {"pipeline": "MinibatchPipeline serves models.Fpt_Boost, not DTW_SVM"}),
    ("params against a DTW_SVM's _X", dict(model=_svm(), params=_p(24)),
     r"barcode_num_events \(24\) must equal the reference length \(25\)", {"pipeline": "MinibatchPipeline serves"}),
    ("refs beside a DTW_SVM", dict(refs=_refs(), model=_svm()), "pass either refs or model", {"pipeline": "MinibatchPipeline serves"}),
    ("DTW_MLP", dict(model=_mlp()), (6, K), {"pipeline": "MinibatchPipeline serves",
                                            "feeder": "Feeder serves models.DTW_SVM and Fpt_Boost, not DTW_MLP"}),
    ("refinement in front of a DTW_SVM", dict(model=_svm(), refine=_refine()), (6, K),
     {"pipeline": "MinibatchPipeline serves", "live": "consensus refinement .* DTW_SVM"}),
]


class _RuleDone(Exception):
    """raised in place of the library: the constructor got past its rule"""


@pytest.mark.parametrize("name,kwargs,expect,own", ROWS, ids=[r[0] for r in ROWS])
def test_one_rule_for_the_three_constructors(monkeypatch, name, kwargs, expect, own):
    def stop(*a, **k):
        raise _RuleDone()

    monkeypatch.setattr(_lib, "load", stop)       # the first thing each constructor does once the rule has passed
    monkeypatch.setattr(_lib, "Context", stop)
    answers = {}
    for who, cls in CLASSES.items():
        obj = cls.__new__(cls)
        if who in own:
            with pytest.raises(ValueError, match=own[who]):
                obj.__init__(**kwargs)
        elif isinstance(expect, tuple):
            with pytest.raises(_RuleDone):
                obj.__init__(**kwargs)
            answers[who] = (obj.nY, obj.K, obj.params.barcode_num_events if "refine" not in kwargs else obj.K)
            assert (obj.nY, obj.K) == expect, who
        else:
            with pytest.raises(ValueError, match=expect) as e:
                obj.__init__(**kwargs)
            answers[who] = str(e.value)
    assert len(set(answers.values())) <= 1, answers      # one rule: the same numbers, the same words
    assert len(answers) + len(own) == len(CLASSES)
