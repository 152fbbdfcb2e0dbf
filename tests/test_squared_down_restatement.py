"""The layer-wise pass behind `HipSquaredCircuit.query_log_marginals` (cirkit_amd/squared_posterior.py) on the host: its
restatement (tests/squared_down_restatement.py) in fp64 reproduces the enumeration for every query set the GPU tests use on the
tiny circuits, in fp32 it stays below a quarter of the bound those tests assert (`R.bound` on the logarithm of the states that
hold at least e^-4 of their row's largest, `S.EPS` in linear space below that: `P.check`), the recorded expectations of the
cases too large to enumerate in a test (tests/golden/sq_posterior_expected.npz) are what recomputing them gives, and the host
plan (`host_plan`) finds the down folds the scope sets give.

Measured (printed by the tests): worst fp64 error 7e-15; worst fp32 error as a fraction of the bound: the tiny circuits 0.003,
as they are and padded to 32 units (cp: 5 of 90 and 5 of 45 states on the linear route, worst linear error 4e-8); 32 signed
units 0.014 (no state on the linear route); the Categorical fixture 0.001 (every state on the logarithm); the hand-built layers
0.003.  Running time: about 90 s, of which 60 s recompute the recorded expectations."""
import numpy as np
import pytest
import torch

import squared_down_restatement as P
import squared_marginal_restatement as R
import squared_sampling_restatement as S


@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_fp64_reproduces_the_enumeration_on_the_tiny_circuits(sum_product):
    plan, tensors, states = R.tiny_case(sum_product)
    x = P.tiny_rows()
    worst = 0.0
    for q, i in P.TINY_QUERIES:
        want = P.expected_query_log_marginals(plan, tensors, x, q, i, states)
        got, ev = P.restated_query_log_marginals(plan, tensors, x, q, i, states, return_evidence=True)
        assert got.shape == (5, len(q), 3)
        worst = max(worst, float((got - want).abs().max()))
        both = R.enumerated_log_marginal(plan, tensors, x, P.mask_of(6, q, i), states)
        worst = max(worst, float((ev - both).abs().max()), float((torch.logsumexp(got, dim=2) - both[:, None]).abs().max()))
    print(f"{sum_product}: worst fp64 error {worst:.2e}")
    assert worst < 1e-11


@pytest.mark.parametrize("padded", [False, True], ids=["3units", "32units"])
@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_fp32_error_of_the_tiny_queries(sum_product, padded):
    plan, tensors, states = R.tiny_case(sum_product)
    x = P.tiny_rows()
    run = R.pad_tiny_to_32(plan, tensors, sum_product) if padded else (plan, tensors)
    for q, i in P.TINY_QUERIES:
        want = P.expected_query_log_marginals(plan, tensors, x, q, i, states)
        if padded:
            assert float((P.restated_query_log_marginals(*run, x, q, i, states) - want).abs().max()) < 1e-11
        got = P.restated_query_log_marginals(*run, x, q, i, states, torch.float32)
        worst, _, _, _ = P.check(got, want, f"tiny {sum_product} padded={padded} Q={q} I={i}")
        assert worst < 0.25


@pytest.mark.parametrize("i", range(len(P.EMB32_QUERIES)))
def test_fp32_error_and_recorded_expectations_of_32_signed_units(i):
    plan, tensors, states = R.emb32_case()
    x = P.emb32_rows()
    q, iv = P.EMB32_QUERIES[i]
    rec = P.golden()[f"emb32_want_{i}"]
    want = P.emb32_expected(i)
    assert rec.shape == (33, len(q), 3) and np.allclose(want, rec, rtol=0, atol=1e-10)
    assert float((P.restated_query_log_marginals(plan, tensors, x, q, iv, states).numpy() - rec).__abs__().max()) < 1e-10
    worst, _, _, _ = P.check(P.restated_query_log_marginals(plan, tensors, x, q, iv, states, torch.float32), rec, f"32 signed units Q={q} I={iv}")
    assert worst < 0.25


def test_fp32_error_and_recorded_expectations_of_the_categorical_fixture():
    plan, tensors, states = R.cat_case()
    q, iv = P.CAT_QUERY
    rec = P.golden()["cat_want"]
    assert rec.shape == (3, 3, 256) and np.allclose(P.cat_expected(), rec, rtol=0, atol=1e-10)
    assert float(np.abs(P.restated_query_log_marginals(plan, tensors, P.cat_rows(), q, iv, states).numpy() - rec).max()) < 1e-9
    worst, _, _, _ = P.check(P.restated_query_log_marginals(plan, tensors, P.cat_rows(), q, iv, states, torch.float32), rec, "categorical fixture",
                             min_log_share=-np.inf)  # (629 of 2304 states lie below e^-4: all held to the bound on the logarithm)
    assert worst < 0.25


@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
def test_fp32_error_of_the_hand_built_layers(cplx):
    """The layers the kernels are run on alone (`P.hand_layer_case`): only the intended all -inf row has no mass, every other
    state holds at least e^-4 of its row's largest, the fp32 restatement of the layer stays below a quarter of the bound."""
    worst = 0.0
    for shape in P.LAYER_SHAPES:
        for B in (1, 3):
            case, Gs, lms, lms32, _ = P.hand_layer_case(cplx, shape, B)
            assert len(lms) == P.LAYER_FOLDS * sum(1 for dn, _ in P.LAYER_SHAPES[shape][4] if dn)
            for k, lm in lms.items():
                worst = max(worst, P.check(lms32[k].expand(B, -1), lm.expand(B, -1), f"{shape} B={B} {k}")[0])
    assert worst < 0.25


def test_host_plan_finds_the_down_folds_and_refuses_a_dag():
    from cirkit_amd.squared_posterior import host_plan
    from cirkit_amd.templates import InputSpec, build_plan, quad_graph

    plan, _, _ = R.emb32_case()
    for q, iv in P.EMB32_QUERIES:
        dp = host_plan(plan, q, P.mask_of(16, q, iv))
        assert dp.down == P.down_folds(plan, q) and dp.top == P.output_fold(plan) and dp.qvars == sorted(q)
        launched = {(dl.layer, f) for dl in dp.layers for f in dl.folds}
        assert launched == {(p, f) for p, f in dp.down if plan.layers[p].inputs is not None}
        assert [dl.layer for dl in dp.layers] == sorted({p for p, _ in launched}, reverse=True)  # the output layer first
        assert dp.mixed.root[0] == R.MIXED if len(q) + len(iv) < 16 else dp.mixed.root[0] == R.INTEGRATED
    dag = build_plan(quad_graph(4, 4), input_layer=InputSpec("embedding", 3), sum_product="cp", num_input_units=2, num_sum_units=2,
                     sum_activation="none", semiring="complex-lse-sum")
    with pytest.raises(NotImplementedError, match="DAG"):
        host_plan(dag, list(range(16)), np.ones(16, dtype=bool))
