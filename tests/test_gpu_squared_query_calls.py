"""What the queries of `HipSquaredCircuit` issue (cirkit_amd/squared.py, squared_sampling.py, squared_posterior.py) against the
`device` section of tests/golden/squared_query_calls.json, recorded on an MI355X by scripts/record_squared_query_calls.py from the
code before the queries shared one fold graph and one child resolver: per case, batch size and query the entry points with their
integer arguments, and a sha256 of every table a squared launch reads -- level, fold and variable rows through the call's own host
pointer, the kind / off / wfold tables of the mixed launches read back -- with arena offsets as they are.  Cases: the tiny circuits
at K = 3 and padded to 32, the 32-unit circuit at 1 and 33 rows (every query, both sampling orders, a conditional sample), in two
chunks and with four rows per workgroup, the Categorical fixture, `log_marginal` of the Gaussian fixture.  No more runs than the
recorder ran."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT

_spec = importlib.util.spec_from_file_location("record_squared_query_calls", os.path.join(ROOT, "scripts", "record_squared_query_calls.py"))
rsq = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rsq)

with open(os.path.join(GOLDEN, "squared_query_calls.json"), encoding="utf-8") as _f:
    DEVICE = json.load(_f)["device"]


def test_fixture_holds_every_case():
    assert set(DEVICE) == set(rsq.device_cases())


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(DEVICE))
def test_queries_issue_the_recorded_calls_over_the_recorded_tables(hip_device, case):
    got, want = rsq.record_device_case(rsq.device_cases()[case], hip_device), DEVICE[case]
    torch.cuda.synchronize()
    assert set(got) == set(want), case
    for B in want:
        assert set(got[B]) == set(want[B]), (case, B)
        for query in want[B]:
            for k in ("calls", "tables", "launches"):
                assert got[B][query][k] == want[B][query][k], (case, B, query, k)
