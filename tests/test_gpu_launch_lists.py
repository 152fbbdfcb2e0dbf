"""The launches `HipCircuit` records and profiles, pinned entry point by entry point (tests/golden/launch_lists.json, written
by scripts/record_launch_lists.py): the forward's launch list, the one of `log_likelihood_sum`, their lengths, whether the
binding reads the caller's batch and evaluates the next forward's parameters, and what `profile_kernels` times -- so that
bench.py's roofline and a recorded forward cannot drift apart unnoticed."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_case

_spec = importlib.util.spec_from_file_location("record_launch_lists", os.path.join(ROOT, "scripts", "record_launch_lists.py"))
rll = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rll)

with open(rll.FIXTURE, encoding="utf-8") as _f:
    _DOC = json.load(_f)
_CASES = {cid: (n, B, v) for cid, n, B, v in rll.all_cases(rll.plan_names()) if cid in _DOC["cases"]}

pytestmark = pytest.mark.gpu


def test_the_fixture_holds_the_cases_the_script_records():
    assert sorted(_CASES) == sorted(_DOC["cases"])
    want = {f"{n}@{rll.LARGE_BATCH}" for n in rll.LARGE} | {f"{n}@{rll.BATCH}[{v}]" for n in rll.VARIED for v in rll.VARIANTS}
    assert want <= set(_CASES)
    assert not set(_DOC["refused"]) & {n for n, _, _ in _CASES.values()}


@pytest.mark.parametrize("cid", sorted(_DOC["cases"]))
def test_launch_lists_match_the_recording(hip_device, cid):
    name, B, variant = _CASES[cid]
    got = rll.record_case(rll.build_circuit(name, variant, hip_device), B)
    want = _DOC["cases"][cid]
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key


@pytest.mark.parametrize("name", ["cfg2_qt784", "cfg4_pd784"])
def test_profiling_leaves_the_forward_bit_identical(hip_device, name):
    from cirkit_amd.circuit import HipCircuit

    plan, tensors, g = load_case(name)
    rows = g["x"][np.arange(64) % len(g["x"])]  # 64 rows: the golden batch, repeated where it is shorter
    x = torch.from_numpy(rows.astype(np.int64 if np.issubdtype(rows.dtype, np.integer) else np.float32)).to(hip_device)
    hc = HipCircuit(plan, tensors, device=hip_device)
    before = hc.forward(x).clone()
    hc.profile_kernels(x, iters=1)
    after = hc.forward(x).clone()
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))
