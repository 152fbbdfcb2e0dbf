"""The job graph and the launch cost model of the training step's job form (cirkit_amd/job_graph.py, job_layout.py) against
what the code they were split out of computed: tests/golden/job_graphs.json (scripts/record_job_graphs.py) and
tests/golden/job_layouts.json (scripts/record_job_layouts.py).  No device and no library: the layers are built on the CPU.

The GPU tests of the job form compare gradients within noise bounds; a wrong level, a lost gradient source or a changed row
split passes those and only shows as a slower step.  Here every job, list, level and split is compared exactly.

No template reaches an input layer that no job epilogue covers (`JobStep._uncovered()` is empty in every case; the recording
script refuses to write a fixture otherwise), so that path has no case here."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rjg = _script("record_job_graphs")
rjl = _script("record_job_layouts")

with open(os.path.join(GOLDEN, "job_graphs.json"), encoding="utf-8") as _f:
    GRAPHS = json.load(_f)
with open(os.path.join(GOLDEN, "job_layouts.json"), encoding="utf-8") as _f:
    LAYOUTS = json.load(_f)


def test_fixture_holds_every_case():
    assert set(GRAPHS["full"]) == set(rjg.FULL) and set(GRAPHS["digest"]) == set(rjg.FULL) | set(rjg.DIGEST)
    assert set(GRAPHS["refused"]) == set(rjg.REFUSED)


@pytest.mark.parametrize("name", list(rjg.FULL) + list(rjg.DIGEST))
def test_job_graph_is_the_recorded_one(name):
    """Counts and the sha256 of the canonical form; for the small circuits the canonical form itself, part by part, so that a
    difference names the job."""
    canon = rjg.case_canonical(name)
    assert rjg.uncovered(canon) == []
    if name in rjg.FULL:
        want = GRAPHS["full"][name]
        got = json.loads(json.dumps(canon))  # (tuples and int keys as the file holds them)
        assert set(got) == set(want)
        for part in want:
            if isinstance(want[part], list) and part.endswith("_jobs"):
                assert len(got[part]) == len(want[part]), part
                for n, (a, b) in enumerate(zip(got[part], want[part])):
                    assert a == b, (part, n)
            else:
                assert got[part] == want[part], part
    assert rjg.digest(canon) == GRAPHS["digest"][name]


def test_recorded_counts_are_the_known_ones():
    """Anchors: the fixture is the one of the circuits it names."""
    d = GRAPHS["digest"]
    count = lambda n: (d[n]["sum_jobs"], d[n]["mix_jobs"], d[n]["folded_mix_jobs"], d[n]["nsum_jobs"], d[n]["gsum_jobs"], d[n]["root_folds"])
    assert count("quadgraph_cat_3x4x4") == (60, 4, 4, 0, 0, 2)
    assert count("pd_gauss_3x4x4") == (400, 59, 59, 0, 85, 6)
    assert count("quadtree_cat_3x4x4") == (30, 0, 0, 0, 0, 1)
    assert count("quadgraph_cat_8x8")[:2] == (252, 20) and count("quadtree_cat_8x8")[:2] == (126, 0)
    assert count("pd_gauss_8x8")[:2] == (12096, 1119) and d["pd_gauss_8x8"]["gsum_jobs"] == 1217
    assert count("cfg4_pd784")[0] == 6272 and d["cfg4_pd784"]["nsum_jobs"] == 49
    assert count("pd_gauss_6x6_k64[fold_mix_bwd=False]")[1:3] == (344, 0) and d["pd_gauss_6x6_k64[fold_mix_bwd=False]"]["gsum_jobs"] == 60
    assert d["quadtree4_cat_8x8[max_list=2]"]["nsum_jobs"] == 21


@pytest.mark.parametrize("name", list(rjg.REFUSED))
def test_refusal_reason_is_the_recorded_one(name):
    source, switches = rjg.REFUSED[name]
    assert rjg.job_graph(source, **switches) == GRAPHS["refused"][name]


def test_refusal_reasons_are_the_known_ones():
    r = GRAPHS["refused"]
    assert r["cfg2_qt784"] == "layer 0: Categorical layers need 64 units and probs = softmax(tensor)"
    assert r["quadgraph_6x6[use_mixing_weights=False]"] == "layer 4: weight parameterisation ['tensor', 'tensor', 'softmax', 'softmax', 'matmul']"
    assert r["quadgraph_6x6[sum_weight_activation=sigmoid]"] == "layer 1: a sum layer of 64 -> 64 units, arity 1, weight ['tensor', 'sigmoid']"
    assert r["quadgraph_6x6[num_classes=3]"] == "layer 14: a cpt layer of 64 -> 3 units, arity 2, weight ['tensor', 'softmax']"


def test_cost_model_returns_the_recorded_layouts():
    from cirkit_amd.job_layout import mix_split, sum_layout

    want = LAYOUTS
    assert want == rjl.record()  # the script's own copy of the arithmetic still records this fixture
    got = rjl.record(sum_layout, mix_split)
    assert len(got["sum"]) == len(want["sum"]) == 364 and len(got["mix"]) == len(want["mix"]) == 100
    for a, b in zip(got["sum"] + got["mix"], want["sum"] + want["mix"]):
        assert a == b, (a, b)
    # the grid reaches both of the model's special answers
    assert any(len(r[4]) > 1 for r in want["sum"]) and any(r[5] == 8 for r in want["sum"])
    # (the example of `sum_layout`'s docstring: 1060 jobs on 512 slots are two rounds of whole jobs + 36 jobs in 8 pieces each)
    assert [r[4:] for r in want["sum"] if r[:4] == [1060, 32, 256, 1]] == [[[[1, 1024], [8, 36]], 4]]
