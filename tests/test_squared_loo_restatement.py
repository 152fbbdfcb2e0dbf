"""The leave-one-out pass of squared circuits on the CPU (tests/squared_loo_restatement.py): its fp64 run against the enumeration,
its fp32 run -- the rounding the GPU kernels can be held to -- against HALF the bounds tests/test_squared_leave_one_out.py asserts
on the GPU (a factor of two for the kernels' different order of sums), and the host plan of cirkit_amd/squared_loo.py.

Measured, fp32, worst error as a fraction of the log bound (unnormalised table / table normalised over the states / per-entry
conditionals): 32 signed units 0.03 / 0.33 / 0.29 with 12 % of the states on the linear route (worst linear error 1.2e-6), the
tiny circuits 0.011 / 0.044 / 0.012, the Categorical fixture 0.002 / 0.060 / 0.028 with every state held to the log bound, the
hand-built layers 0.032."""
import functools

import pytest
import torch

import squared_down_restatement as P
import squared_loo_restatement as L
import squared_marginal_restatement as R
import squared_sampling_restatement as S


@functools.lru_cache(maxsize=None)
def _case(name):
    plan, tensors, states, rows, queries, share = L.cases()[name]
    allv = list(range(plan.num_variables))
    return plan, tensors, states, rows, queries, share, L.expected_loo_log_marginals(plan, tensors, rows, allv, states)


CASES = ["tiny-cp-3", "tiny-cp-32", "tiny-cp-t-3", "tiny-cp-t-32", "emb32", "cat"]


@pytest.mark.parametrize("name", CASES)
def test_fp64_reproduces_the_enumeration(name):
    plan, tensors, states, rows, queries, _, want = _case(name)
    for q in queries:
        got = L.restated_loo_log_marginals(plan, tensors, rows, q, states)
        err = float((got - want[:, q]).abs().max())
        print(f"{name} Q={q}: fp64 against the enumeration {err:.1e}")
        assert got.shape == (rows.shape[0], len(q), states) and err <= 1e-11
    allv = list(range(plan.num_variables))
    got = L.restated_loo_log_marginals(plan, tensors, rows, allv, states)
    at_x = L.entries(got, rows, allv)
    log_c2 = R.log_c2_of(plan, tensors, rows)
    err = float((at_x - log_c2[:, None]).abs().max())
    print(f"{name}: the observed state against 2 Re log c {err:.1e}")
    assert err <= 1e-11


@pytest.mark.parametrize("name", CASES)
def test_fp32_stays_within_half_the_bounds(name):
    """Half of what the GPU test asserts, on the unnormalised table, the table normalised over the states and the per-entry
    conditionals; the cap on the linear route (a quarter of the states, of the entries) is asserted by the checks themselves."""
    plan, tensors, states, rows, _, share, want = _case(name)
    allv = list(range(plan.num_variables))
    got = L.restated_loo_log_marginals(plan, tensors, rows, allv, states, torch.float32)
    assert got.dtype == torch.float32
    for what, g, w in (("unnormalised", got, want), ("normalised", L.normalise(got), L.normalise(want))):
        wl, wlin, _, _ = P.check(g, w, f"{name} {what}", min_log_share=share)
        assert wl <= 0.5 and wlin <= 0.5 * S.EPS
    wl, wlin, _, _ = L.check_entries(L.entries(L.normalise(got), rows, allv), L.entries(L.normalise(want), rows, allv), f"{name} entries", share)
    assert wl <= 0.5 and wlin <= 0.5 * S.EPS


@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
@pytest.mark.parametrize("shape", list(L.LAYER_SHAPES))
def test_hand_layers_hold_their_edges(shape, cplx):
    """What the kernel tests rely on: the zero weight column is a -inf unit of every written D, the all -inf row stays -inf (no
    NaN), and the fp32 run of a layer stays within half of `S.EPS` of the fp64 one."""
    for B in (1, 35):
        case = L.hand_layer(cplx, shape, B)
        Ds, lms = L.hand_layer_run(case)
        Ds32, lms32 = L.hand_layer_run(case, torch.float32)
        for d64, d32 in zip(Ds, Ds32):
            for h, d in d64.items():
                re = d.real if cplx else d
                assert not torch.isnan(re).any()
                if case["w"] is not None:
                    assert bool(torch.isneginf(re[:, -1]).all())
                if B > 1 and not case["top"]:
                    assert bool(torch.isneginf(re[B - 1]).all())
                assert L.linear_error(d32[h].to(torch.complex128 if cplx else torch.float64).numpy(), d.numpy()) <= 0.5 * S.EPS
        for k, lm in lms.items():
            lm = lm.expand(B, -1)
            assert not torch.isnan(lm).any()
            if B > 1 and not case["top"]:
                assert bool(torch.isneginf(lm[B - 1]).all()) and bool(torch.isfinite(lm[: B - 1]).all())
        want = torch.stack([lms[k].expand(B, -1) for k in sorted(lms)], dim=1)
        got = torch.stack([lms32[k].expand(B, -1) for k in sorted(lms)], dim=1)
        live = slice(0, B - 1) if B > 1 and not case["top"] else slice(0, B)
        for what, g, w in (("log m", got, want), ("normalised", L.normalise(got[live]), L.normalise(want[live]))):
            wl, wlin, _, _ = P.check(g, w, f"{shape} B={B} {what}")
            assert wl <= 0.5 and wlin <= 0.5 * S.EPS


# ---- the host plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [[3], [0, 1, 4], list(range(6))])
def test_host_plan_against_scope_sets(q):
    from cirkit_amd.squared_loo import host_plan

    plan, _, _ = R.tiny_case("cp")
    lp = host_plan(plan, q)
    assert lp.qvars == sorted(q) and lp.down == P.down_folds(plan, q) and lp.top == P.output_fold(plan)
    scopes = R.fold_scopes(plan)
    assert [scopes[p][f] for p, f in lp.leaves] == [frozenset([v]) for v in sorted(q)]
    order = [ll.layer for ll in lp.layers]
    assert order == sorted(order, reverse=True) and order[0] == lp.top[0]  # the output layer first, every layer once
    want = {p for p, f in lp.down if plan.layers[p].inputs is not None}
    assert set(order) == want and len(order) == len(want)
    for ll in lp.layers:
        assert ll.folds == sorted(f for p, f in lp.down if p == ll.layer)
        assert ll.children.shape == (len(ll.folds), plan.layers[ll.layer].arity, 2)
        for f, ch in zip(ll.folds, ll.children.tolist()):  # a down fold has a down child: its query variable lies below one
            assert any((p, g) in lp.down for p, g in ch)
            assert frozenset().union(*(scopes[p][g] for p, g in ch)) == scopes[ll.layer][f]
    _, launch_order = L.derivatives(plan, *_tiny_inputs(), q, torch.float64)
    assert [(ll.layer, ll.folds) for ll in lp.layers] == launch_order


def _tiny_inputs():
    return R.tiny_case("cp")[1], P.tiny_rows()


def test_host_plan_refusals():
    from cirkit_amd.squared_loo import host_plan
    from cirkit_amd.templates import InputSpec, build_plan, quad_graph

    plan, _, _ = R.gauss_case()
    with pytest.raises(NotImplementedError, match="Gaussian"):
        host_plan(plan, [1, 2])
    dag = build_plan(quad_graph(4, 4), input_layer=InputSpec("embedding", 3), sum_product="cp", num_input_units=4, num_sum_units=4,
                     sum_activation="none", semiring="complex-lse-sum")
    with pytest.raises(NotImplementedError, match="DAG"):
        host_plan(dag, [5, 6])
    with pytest.raises(ValueError, match="at least one"):
        host_plan(R.tiny_case("cp")[0], [])
