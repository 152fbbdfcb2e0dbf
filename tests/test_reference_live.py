"""Further circuits compiled by the real reference, beyond the BASELINE fixtures: the reference's outputs on them are
recorded under tests/golden/live_* (tests/golden/make_fixtures.py:reference_live, which compiles each circuit with
april-tools/cirkit itself and stores its folded plan, its own random parameters, the inputs and its outputs).  Checks that
(1) the native plan builder emits the reference's folded plan, (2) the oracle reproduces the reference's forward bit for bit
with the same parameters, and (3) the natively built partition function of a squared circuit equals the reference's
`integrate(multiply(c, c))`."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_case
from cirkit_amd.functional import squared_partition_plan
from cirkit_amd.templates import image_data
from oracle.torch_oracle import as_torch, evaluate_plan
from test_templates import _assert_same_plan

CASES = [
    ((1, 5, 4), "quad-graph", "categorical", "cp", 3, 1, True),
    ((1, 6, 6), "quad-tree-4", "categorical", "tucker", 2, 1, True),
    ((2, 4, 4), "quad-tree-2", "gaussian", "cp-t", 3, 1, True),
    ((1, 8, 8), "poon-domingos", "gaussian", "cp", 2, 1, True),
    ((1, 4, 6), "random-binary-tree", "binomial", "cp", 3, 1, True),
    ((1, 6, 6), "quad-graph", "categorical", "cp", 3, 4, False),
    ((1, 7, 5), "poon-domingos", "binomial", "cp-t", 2, 1, True),
]


def _x(g):
    x = g["x"]
    return torch.from_numpy(x if x.dtype.kind == "f" else x.astype(np.int64))


@pytest.mark.parametrize("shape,rg,inp,sp,k,ncls,mix", CASES, ids=[f"{c[1]}-{c[2]}-{c[3]}" for c in CASES])
def test_plan_and_forward_match_the_live_reference(shape, rg, inp, sp, k, ncls, mix):
    plan, tensors, g = load_case(f"live_fwd{CASES.index((shape, rg, inp, sp, k, ncls, mix))}")
    kw = dict(input_layer=inp, num_input_units=k, sum_product_layer=sp, num_sum_units=k, num_classes=ncls, use_mixing_weights=mix)
    _assert_same_plan(image_data(shape, rg, **kw), plan)
    got = evaluate_plan(plan, as_torch(tensors), _x(g))
    assert got.shape == g["y"].shape and np.array_equal(got.numpy(), g["y"])


@pytest.mark.parametrize("activation,native", [("softplus", "softplus"), ("positive-clamp", "positive-clamp"), ("sigmoid", "sigmoid")])
def test_sum_weight_activations_match_the_live_reference(activation, native):
    """The sum-weight activations templates/utils.py name_to_parameter_activation names beside softmax (:185-194): the natively
    built plan is the reference's (TorchSoftplusParameter / TorchClampParameter with vmin = 1e-18 / TorchSigmoidParameter nodes)
    and the oracle reproduces the reference's forward bit for bit."""
    plan, tensors, g = load_case(f"live_act{['softplus', 'positive-clamp', 'sigmoid'].index(activation)}")
    _assert_same_plan(image_data((1, 4, 4), "quad-tree-2", input_layer="categorical", num_input_units=3, sum_product_layer="cp",
                                 num_sum_units=3, sum_weight_activation=native), plan)
    got = evaluate_plan(plan, as_torch(tensors), _x(g))
    assert got.shape == g["y"].shape and np.array_equal(got.numpy(), g["y"])


@pytest.mark.parametrize("inp", ["categorical", "gaussian"])
def test_squared_partition_function_matches_the_live_reference(inp):
    plan, tensors, g = load_case(f"live_sq{['categorical', 'gaussian'].index(inp)}")
    want = float(g["z"].reshape(-1)[0])
    got = float(evaluate_plan(squared_partition_plan(plan), as_torch(tensors), None).reshape(-1)[0])
    assert abs(got - want) <= 1e-5 * abs(want)


def test_complex_squared_circuit_matches_the_live_reference():
    """Embedding inputs, unconstrained weights, complex-lse-sum: c(x) through the oracle and Z built natively."""
    plan, tensors, g = load_case("live_complex_sq")
    _assert_same_plan(image_data((1, 4, 4), "quad-tree-2", input_layer="embedding", num_input_units=3, sum_product_layer="cp-t",
                                 num_sum_units=3, sum_weight_activation="none", semiring="complex-lse-sum"), plan)
    tens = as_torch(tensors)
    y = evaluate_plan(plan, tens, _x(g))
    assert y.shape == g["y"].shape and np.array_equal(y.numpy(), g["y"])
    want = g["z"].reshape(-1)[0]
    got = evaluate_plan(squared_partition_plan(plan), tens, None).reshape(-1)[0]
    assert abs(float(got.real) - float(want.real)) <= 1e-5 * abs(float(want.real))


PARAM_NODE_CASES = [
    ("TorchHadamardParameter", {}, [(3, 5), (3, 5)], "hadamard", {}),
    ("TorchKroneckerParameter", {}, [(2, 3), (4, 5)], "kronecker", {}),
    ("TorchOuterProductParameter", {"dim": 1}, [(3, 2), (3, 4)], "outer_product", {"dim": 1}),
    ("TorchReduceSumParameter", {"dim": 0}, [(4, 2, 3)], "reduce_sum", {"dim": 0}),
    ("TorchSumParameter", {}, [(4, 3), (4, 3)], "sum", {}),
    ("TorchReduceProductParameter", {"dim": 1}, [(3, 6)], "reduce_prod", {"dim": 1}),
    ("TorchReduceLSEParameter", {"dim": 0}, [(4, 2, 3)], "reduce_lse", {"dim": 0}),
    ("TorchOuterSumParameter", {"dim": 1}, [(3, 2), (3, 4)], "outer_sum", {"dim": 1}),
    ("TorchIndexParameter", {"indices": [2, 0, 2, 4], "dim": 0}, [(5, 3)], "index", {"indices": [2, 0, 2, 4], "dim": 0}),
    ("TorchGaussianProductMean", {}, [(4, 1), (4, 1), (3, 1), (3, 1)], "gaussian_product_mean", {}),
    ("TorchGaussianProductStddev", {}, [(4, 1), (3, 1)], "gaussian_product_stddev", {}),
    ("TorchClampParameter", {"vmin": 1e-18}, [(5, 7)], "clamp", {"vmin": 1e-18}),
    ("TorchClampParameter", {"vmin": -0.3, "vmax": 0.4}, [(5, 7)], "clamp", {"vmin": -0.3, "vmax": 0.4}),
    ("TorchSoftplusParameter", {}, [(5, 7)], "softplus", {}),
]


@pytest.mark.parametrize("cls,kwargs,shapes,op,config", PARAM_NODE_CASES)
def test_oracle_parameter_nodes_equal_the_reference_modules(cls, kwargs, shapes, op, config):
    """The oracle's restatement of the parameter nodes added in round 6 (nodes.py:491-612, 702-751) against the outputs of the
    reference's own modules on the same operands: bit for bit, and the plan extraction maps each class to its op."""
    from cirkit_amd.plan import IDX_NONE, PARAM_OPS, FoldIndex, ParamGraph, ParamNode
    from oracle.torch_oracle import eval_param

    assert PARAM_OPS[cls] == op
    F = 3
    i = PARAM_NODE_CASES.index((cls, kwargs, shapes, op, config))
    with np.load(os.path.join(GOLDEN, "live_param_nodes.npz")) as z:
        xs = [torch.from_numpy(z[f"c{i}_x{j}"]) for j in range(len(shapes))]
        want = torch.from_numpy(z[f"c{i}_want"])
        out_shape = tuple(int(s) for s in z[f"c{i}_shape"])
    assert [tuple(x.shape) for x in xs] == [(F, *s) for s in shapes]
    nodes = [ParamNode("tensor", F, tuple(s), {"tensor": f"t{i}"}, []) for i, s in enumerate(shapes)]
    nodes.append(ParamNode(op, F, out_shape, dict(config), [FoldIndex([i], IDX_NONE) for i in range(len(shapes))]))
    pg = ParamGraph(nodes, FoldIndex([len(nodes) - 1], IDX_NONE), F, out_shape)
    got = eval_param(pg, {f"t{i}": x for i, x in enumerate(xs)})
    assert got.shape == want.shape and torch.equal(got, want)
