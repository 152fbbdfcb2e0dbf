"""What the job form of the training step binds and records (cirkit_amd/train_jobs.py) against tests/golden/job_step_calls.json,
recorded on an MI355X by scripts/record_job_step_calls.py from the code before the job graph, the cost model and the binding
were split: per case and mode the entry points the recorded program issues with their count arguments (units, waves, hmax,
block size, B, C), a sha256 of every job launch's device table (pointer fields reduced to zero / non-zero), the pool's length and
the number of extra blocks.  No step runs."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT

_spec = importlib.util.spec_from_file_location("record_job_step_calls", os.path.join(ROOT, "scripts", "record_job_step_calls.py"))
rjs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rjs)

with open(os.path.join(GOLDEN, "job_step_calls.json"), encoding="utf-8") as _f:
    FIXTURE = json.load(_f)


def test_fixture_holds_every_case():
    want = {f"{c}@{B}/mode{m}" for c, (_, _, _, batches) in rjs.CASES.items() for B in batches for m in (1, 2)}
    assert set(FIXTURE["cases"]) == want


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rjs.CASES))
def test_bound_step_issues_the_recorded_calls_over_the_recorded_tables(hip_device, case):
    tr = rjs.make_trainer(case, hip_device)
    if int(tr.circuit._n_cu) != FIXTURE["n_cu"]:
        pytest.skip(f"the fixture was recorded on a device with {FIXTURE['n_cu']} CUs, this one has {tr.circuit._n_cu}: the row splits differ")
    for B in rjs.CASES[case][3]:
        for mode in (1, 2):
            cid = f"{case}@{B}/mode{mode}"
            got = json.loads(json.dumps(rjs.record_case(tr, B, mode)))
            want = FIXTURE["cases"][cid]
            assert got["calls"] == want["calls"], cid
            assert [k for k, _ in got["tables"]] == [k for k, _ in want["tables"]], cid
            for n, (a, b) in enumerate(zip(got["tables"], want["tables"])):
                assert a == b, (cid, n, a[0])
            assert {k: got[k] for k in ("num_ops", "pool", "n_extra")} == {k: want[k] for k in ("num_ops", "pool", "n_extra")}, cid
    torch.cuda.synchronize()
