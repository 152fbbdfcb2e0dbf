"""Chow-Liu structure learning on the host (cirkit_amd/structure.py, cirkit_amd/templates.py): the fp64 restatement and the
restored host path return the trees the reference learned from the committed datasets, `tabular_data('chow-liu-tree',
data=...)` emits the plans the reference compiled from them, and the refusals that need no device."""
import os

import numpy as np
import pytest
import torch

from chow_liu_restatement import chain_cases, edges_of, mutual_information, tree_of
from conftest import GOLDEN
from cirkit_amd.plan import Plan
from cirkit_amd.structure import chow_liu_predecessors, pairwise_mutual_information
from cirkit_amd.templates import tabular_data, tree_to_region_graph
from test_templates import _assert_same_plan

# the arguments of tests/golden/make_fixtures.py::chow_liu
CASES = {
    "plan_clt_cat9_cp": ({"name": "categorical", "args": {"num_categories": 4}}, "cp"),
    "plan_clt_gauss7_cpt": ({"name": "gaussian", "args": {}}, "cp-t"),
    "plan_clt_mixed6_cp": ([{"name": "categorical", "args": {"num_categories": 3}}, {"name": "gaussian", "args": {}}] * 3, "cp"),
}


def _dataset(name):
    with np.load(os.path.join(GOLDEN, name + "_data.npz")) as z:
        return z["data"], z["tree"]


def test_restatement_returns_the_committed_categorical_tree():
    data, tree = _dataset("plan_clt_cat9_cp")
    mi = mutual_information(data, 4)
    assert np.abs(mi - mi.T).max() <= 1e-14 and not mi.diagonal().any()  # (symmetric up to the order of its fp64 sums)
    assert np.array_equal(tree_of(mi), tree)
    assert list(tree) == [7, 8, 4, -1, 3, 6, 1, 2, 3]


def test_restatement_recovers_the_noisy_chains():
    for _, x, edges in chain_cases():
        assert edges_of(tree_of(mutual_information(x))) == edges


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_path_returns_the_committed_trees(name):
    data, tree = _dataset(name)
    inputs, _ = CASES[name]
    itype = inputs["name"] if isinstance(inputs, dict) else [i["name"] for i in inputs]
    ncat = inputs["args"]["num_categories"] if isinstance(inputs, dict) and inputs["name"] == "categorical" else None
    assert np.array_equal(chow_liu_predecessors(torch.from_numpy(data), itype, num_categories=ncat), tree)


@pytest.mark.parametrize("name", sorted(CASES))
def test_tabular_data_reproduces_the_reference_plans(name):
    data, _ = _dataset(name)
    inputs, sp = CASES[name]
    built = tabular_data("chow-liu-tree", data=torch.from_numpy(data), input_layers=inputs, num_input_units=3,
                         sum_product_layer=sp, num_sum_units=3)
    _assert_same_plan(built, Plan.load(os.path.join(GOLDEN, name)))


def test_random_binary_tree_takes_its_width_from_the_data():
    kw = dict(input_layers={"name": "categorical", "args": {"num_categories": 4}}, num_input_units=4, sum_product_layer="cp",
              num_sum_units=4)
    built = tabular_data("random-binary-tree", data=torch.zeros(5, 8, dtype=torch.int64), **kw)
    _assert_same_plan(built, Plan.load(os.path.join(GOLDEN, "cfg1_rbt8")))


def test_chow_liu_without_data_says_what_it_needs():
    with pytest.raises(NotImplementedError, match="data="):
        tabular_data("chow-liu-tree", input_layers={"name": "gaussian", "args": {}}, num_input_units=2, num_sum_units=2)


def test_tree_to_region_graph():
    rg = tree_to_region_graph([1, -1, 1, 2])
    assert rg.scope[rg.root] == (0, 1, 2, 3)
    with pytest.raises(ValueError):
        tree_to_region_graph([-1, 0, -1, 2])  # a forest
    with pytest.raises(ValueError):
        chow_liu_predecessors(torch.zeros(4, 3, dtype=torch.int64), "categorical", root=3)


def test_more_than_2_to_the_24_rows_are_refused_on_the_shape():
    big = torch.zeros(1, 2, dtype=torch.int64).expand(2**24 + 1, 2)  # (a view: nothing is allocated)
    with pytest.raises(ValueError, match="2\\^24"):
        pairwise_mutual_information(big, 2)


def test_the_device_functions_refuse_host_data():
    with pytest.raises(ValueError, match="ROCm device"):
        pairwise_mutual_information(torch.zeros(4, 3, dtype=torch.int64), 2)
