"""What the queries of `HipSquaredCircuit` plan on the host (cirkit_amd/squared_graph.py, `fold_classes` / `mixed_plan` of
cirkit_amd/squared.py, `host_plan` of cirkit_amd/squared_posterior.py) against the `host` section of
tests/golden/squared_query_calls.json, recorded by scripts/record_squared_query_calls.py from the code before the queries shared
one fold graph: per plan `tree_order`, `scope_bits`, the `path_plan` of every variable, and per mask, step and query set the fold
classes, the mixed plan -- plain, with `path=`, with `readers=` -- and the down plan, compared exactly.  No device is needed."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

_spec = importlib.util.spec_from_file_location("record_squared_query_calls", os.path.join(ROOT, "scripts", "record_squared_query_calls.py"))
rsq = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rsq)

with open(os.path.join(GOLDEN, "squared_query_calls.json"), encoding="utf-8") as _f:
    HOST = json.load(_f)["host"]


def test_fixture_holds_every_plan():
    assert set(HOST) == set(rsq.host_cases())


@pytest.mark.parametrize("name", sorted(HOST))
def test_host_plans_are_the_recorded_ones(name):
    got, want = rsq.record_host_case(*rsq.host_cases()[name]), HOST[name]
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], (name, k)
