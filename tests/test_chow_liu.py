"""Chow-Liu structure learning on the GPU (cirkit_amd/structure.py, cirkit_amd/csrc/ck_mi.hip): the pair counts bit for bit
against numpy, the mutual information against the fp64 restatement of the reference's formula
(tests/chow_liu_restatement.py), the learned trees, and a circuit built on a learned plan.

Tolerance of the mutual information: the counts are exact, so the kernel and the restatement differ in fp64 `log` (an ulp
or so of values below 30 in magnitude) and in the order of a sum of at most 65536 terms whose absolute values sum to below
60: about 65536 x 2^-53 x 60 = 4e-10.  The bound is 1e-9 absolute."""
import os

import numpy as np
import pytest
import torch

from chow_liu_restatement import asymmetric_data, chain_cases, edges_of, joint_counts, mutual_information, tree_of
from conftest import GOLDEN
from cirkit_amd.plan import Plan
from cirkit_amd.structure import chow_liu_predecessors, pairwise_counts, pairwise_mutual_information
from cirkit_amd.templates import tabular_data
from test_templates import _assert_same_plan

pytestmark = pytest.mark.gpu
MI_TOL = 1e-9

STATES = [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 40]  # every padded width 2 .. 32, the first padded state, several tiles per pair
ROWS = [1, 15, 16, 17, 257]  # below, at and above one k step of 16 rows; several steps with a ragged last one


def _shapes(c):
    return [(d, n) for d in (2, 3, 9) for n in ROWS] + ([(70, n) for n in ROWS] if c == 2 else [])  # D = 70: ragged last block row


def _check(x: np.ndarray, c: int, device, **kw):
    """Counts bit for bit, MI to MI_TOL, symmetric and repeatable to the bit."""
    xd = torch.from_numpy(x).to(device)
    counts = pairwise_counts(xd, c, **kw).cpu().numpy()
    ref = joint_counts(x, c)
    assert counts.dtype == np.int64 and counts.shape == ref.shape
    assert np.array_equal(counts, ref), f"counts differ at {np.argwhere(counts != ref)[:4].tolist()} (D, N) = {x.shape[::-1]}, C = {c}"
    mi = pairwise_mutual_information(xd, c, **kw)
    assert mi.dtype == torch.float64 and mi.shape == (x.shape[1], x.shape[1])
    assert torch.equal(mi, mi.t()) and not mi.diagonal().any()
    assert torch.equal(mi, pairwise_mutual_information(xd, c, **kw))
    err = float(np.abs(mi.cpu().numpy() - mutual_information(x, c)).max())
    assert err <= MI_TOL, (err, x.shape, c)
    return mi


@pytest.mark.parametrize("c", STATES)
def test_counts_are_exact_and_mi_matches_the_restatement(hip_device, c):
    rng = np.random.default_rng(100 + c)
    for d, n in _shapes(c):
        _check(asymmetric_data(rng, n, d, c), c, hip_device)


@pytest.mark.parametrize("c", [70, 256])  # a pair over 3 x 3 tiles in 2 x 2 blocks of blocks (the last one half empty); 8 x 8 tiles
def test_wide_pairs_walk_all_their_tiles(hip_device, c):
    rng = np.random.default_rng(c)
    _check(asymmetric_data(rng, 257, 3, c), c, hip_device)


@pytest.mark.parametrize("c", [3, 32, 40, 256])
def test_constant_columns(hip_device, c):
    for value in (0, c - 1):
        for n in (17, 257):
            _check(np.full((n, 3), value, dtype=np.int64), c, hip_device)


def test_inputs_int32_missing_num_categories_other_stream(hip_device):
    rng = np.random.default_rng(5)
    x = asymmetric_data(rng, 257, 9, 5)
    x[0, 0] = 4  # (so that max + 1 is 5)
    xd = torch.from_numpy(x).to(hip_device)
    mi = pairwise_mutual_information(xd, 5)
    assert torch.equal(mi, pairwise_mutual_information(xd.to(torch.int32), 5))
    assert torch.equal(mi, pairwise_mutual_information(xd))  # num_categories = max + 1
    assert torch.equal(mi, pairwise_mutual_information(xd.t().contiguous().t(), 5))  # (a strided view)
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):
        other = pairwise_mutual_information(xd, 5)
    side.synchronize()
    assert torch.equal(mi, other)
    alpha = float(np.abs(pairwise_mutual_information(xd, 5, alpha=0.5).cpu().numpy() - mutual_information(x, 5, alpha=0.5)).max())
    assert alpha <= MI_TOL


def test_num_bins_rescales_before_counting(hip_device):
    rng = np.random.default_rng(8)
    x = asymmetric_data(rng, 257, 9, 256)
    xd = torch.from_numpy(x).to(hip_device)
    mi = pairwise_mutual_information(xd, 256, num_bins=8)
    assert float(np.abs(mi.cpu().numpy() - mutual_information(x // 32, 8)).max()) <= MI_TOL
    assert np.array_equal(pairwise_counts(xd, 256, num_bins=8).cpu().numpy(), joint_counts(x // 32, 8))
    with pytest.raises(ValueError):
        pairwise_mutual_information(xd, None, num_bins=8)  # bins of an unknown range


def test_committed_tree_and_plan_from_device_data(hip_device):
    with np.load(os.path.join(GOLDEN, "plan_clt_cat9_cp_data.npz")) as z:
        data, tree = z["data"], z["tree"]
    xd = torch.from_numpy(data).to(hip_device)
    assert np.array_equal(chow_liu_predecessors(xd, "categorical", num_categories=4), tree)
    assert np.array_equal(tree_of(pairwise_mutual_information(xd, 4).cpu().numpy()), tree)
    built = tabular_data("chow-liu-tree", data=xd, input_layers={"name": "categorical", "args": {"num_categories": 4}},
                         num_input_units=3, sum_product_layer="cp", num_sum_units=3)
    _assert_same_plan(built, Plan.load(os.path.join(GOLDEN, "plan_clt_cat9_cp")))


def test_noisy_chains_are_recovered(hip_device):
    for (d, c, n), x, edges in chain_cases():
        pred = chow_liu_predecessors(torch.from_numpy(x).to(hip_device), "categorical")
        assert edges_of(pred) == edges, (d, c, n)


def test_refusals(hip_device):
    x = torch.zeros(20, 3, dtype=torch.int64, device=hip_device)
    bad = x.clone()
    bad[7, 1] = -1
    with pytest.raises(ValueError):
        pairwise_mutual_information(bad, 4)
    with pytest.raises(ValueError):
        pairwise_mutual_information(bad)  # (max + 1 does not hide it)
    bad[7, 1] = 4
    with pytest.raises(ValueError):
        pairwise_mutual_information(bad, 4)
    with pytest.raises(ValueError):
        pairwise_counts(bad, 4)
    with pytest.raises(ValueError):
        chow_liu_predecessors(bad, "categorical", num_categories=4)
    with pytest.raises(ValueError):
        pairwise_mutual_information(x, 257)
    with pytest.raises(ValueError):
        pairwise_mutual_information(x.double(), 4)
    with pytest.raises(ValueError, match="2\\^28"):
        pairwise_counts(torch.zeros(4, 70, dtype=torch.int64, device=hip_device), 256)
    assert torch.isfinite(pairwise_mutual_information(x, 4)).all()  # (a refusal leaves nothing behind)


def test_circuit_on_a_learned_plan_matches_the_oracle(hip_device):
    """The bound of test_gpu_parity.py::test_chow_liu_circuits_match_oracle."""
    from cirkit_amd.circuit import HipCircuit
    from cirkit_amd.initializers import init_plan_tensors
    from oracle.torch_oracle import as_torch, evaluate_plan

    with np.load(os.path.join(GOLDEN, "plan_clt_cat9_cp_data.npz")) as z:
        x = torch.from_numpy(z["data"])
    plan = tabular_data("chow-liu-tree", data=x.to(hip_device), input_layers={"name": "categorical", "args": {"num_categories": 4}},
                        num_input_units=3, sum_product_layer="cp", num_sum_units=3)
    tensors = init_plan_tensors(plan, seed=9)
    want = evaluate_plan(plan, as_torch(tensors), x)
    got = HipCircuit(plan, tensors, device=hip_device)(x.to(hip_device)).cpu()
    assert got.shape == want.shape and torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
