"""What the fused, the layer-wise and the signed squared training steps bind and issue (cirkit_amd/train_fused.py,
cirkit_amd/training.py, cirkit_amd/training_squared.py) against tests/golden/train_step_calls.json, recorded on an MI355X by
scripts/record_train_calls.py from the code before the fused form moved out of `HipTrainer`: per case the entry points issued
with their count arguments (those of every `LeafBwdLaunch`, whether `ck_table_dense_bwd` got a `TableOpt`), a sha256 of every
host-built table (pointer fields reduced to zero / non-zero), shapes, flags.  No more runs than the recorder ran.

tests/golden/squared_step_calls.json holds the same for the other paths of `HipSquaredTrainer` (cirkit_amd/train_reverse.py,
cirkit_amd/train_signed.py), recorded from the code before the trainer was split: the complex and the real layer-wise lists with
both Embedding branches, Categorical and Gaussian inputs, the signed circuit without its leaf region, the `step` form and a second
global batch; beside the calls the weight-pool layout, the scratch shapes and the table digests of c and of Z."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT

_spec = importlib.util.spec_from_file_location("record_train_calls", os.path.join(ROOT, "scripts", "record_train_calls.py"))
rtc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rtc)

with open(os.path.join(GOLDEN, "train_step_calls.json"), encoding="utf-8") as _f:
    FIXTURE = json.load(_f)
with open(os.path.join(GOLDEN, "squared_step_calls.json"), encoding="utf-8") as _f:
    SQUARED = json.load(_f)


def _same_device(tr_n_cu) -> None:
    if int(tr_n_cu) != FIXTURE["n_cu"]:
        pytest.skip(f"the fixture was recorded on a device with {FIXTURE['n_cu']} CUs, this one has {tr_n_cu}: the work segments differ")


def _compare(got: dict, want: dict, cid: str) -> None:
    got = json.loads(json.dumps(got))
    assert set(got) == set(want), cid
    for k in want:
        assert got[k] == want[k], (cid, k)


def test_fixture_holds_every_case():
    assert set(FIXTURE["fused"]) == {f"{c}@{B}" for c, (_, _, batches, _) in rtc.FUSED_CASES.items() for B in batches}
    assert set(FIXTURE["unit_tabs"]) == set(rtc.FUSED_CASES)
    assert set(FIXTURE["layerwise"]) == {f"{c}@{B}" for c in rtc.LAYERWISE_CASES for B in rtc.LAYERWISE_BATCHES}
    assert FIXTURE["signed"]["calls"]
    assert set(SQUARED["squared"]) == {f"{c}@{B}" for c, cfg in rtc.SQUARED_CASES.items() for B in cfg[5]}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rtc.FUSED_CASES))
def test_fused_step_issues_the_recorded_calls_over_the_recorded_tables(hip_device, case):
    tr = rtc.make_fused(case, hip_device)
    _same_device(tr.circuit._n_cu)
    assert json.loads(json.dumps(rtc.unit_table_digests(tr))) == FIXTURE["unit_tabs"][case]
    for B in rtc.FUSED_CASES[case][2]:
        _compare(rtc.record_fused(tr, case, B), FIXTURE["fused"][f"{case}@{B}"], f"{case}@{B}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rtc.LAYERWISE_CASES))
def test_layerwise_backward_issues_the_recorded_calls_over_the_recorded_tables(hip_device, case):
    tr = rtc.make_layerwise(case, hip_device)
    for B in rtc.LAYERWISE_BATCHES:
        _compare(rtc.record_layerwise(tr, B), FIXTURE["layerwise"][f"{case}@{B}"], f"{case}@{B}")


@pytest.mark.gpu
def test_signed_squared_step_issues_the_recorded_calls_over_the_recorded_tables(hip_device):
    tr = rtc.make_signed(hip_device)
    _same_device(tr._signed.c._n_cu)
    _compare(rtc.record_signed(tr), FIXTURE["signed"], "signed")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(rtc.SQUARED_CASES))
def test_squared_trainer_issues_the_recorded_calls_over_the_recorded_state(hip_device, case):
    """(No work segments enter these lists: they hold on any number of CUs.)"""
    tr = rtc.make_squared(case, hip_device)
    for B in rtc.SQUARED_CASES[case][5]:
        _compare(rtc.record_squared(tr, case, B), SQUARED["squared"][f"{case}@{B}"], f"{case}@{B}")
    torch.cuda.synchronize()
