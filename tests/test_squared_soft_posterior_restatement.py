"""The passes behind `HipSquaredCircuit.soft_query_log_marginals`, `soft_posterior_marginals` and `sample_soft`
(cirkit_amd/squared_soft_posterior.py) on the host: the restatement (tests/squared_soft_posterior_restatement.py) in fp64
reproduces the enumeration on the tiny circuits for every subset of `RS.TINY_VARS`, with and without `RS.TINY_OTHER` integrated,
and for S = all; in fp32 it stays below half the bound the GPU tests assert (`P.check`, which also asserts that at most a quarter
of a case's finite states take the linear route: the share is checked here, on the host); the recorded expectations
(tests/golden/sq_soft_posterior_expected.npz) are what recomputing them gives; the host plan finds the down folds, reads the leaf
Gram blocks as FULL children and leaves plans without soft variables as they were; the sibling rule of `sample_soft` refuses a
raster order and needs no soft re-evaluation in `tree_order`; every refusal of the planning layer.

Measured (printed by the tests): worst fp64 error 4.5e-12; worst fp32 error as a fraction of HALF the GPU bound, the limit asserted: the tiny
circuits 0.073, 32 signed units 0.076 (one soft pixel: 15 of 82 states on the linear route, worst linear error 2.7e-6), the Categorical fixture
0.003.  Running time: about 15 s."""
import types

import numpy as np
import pytest
import torch

import squared_down_restatement as P
import squared_marginal_restatement as R
import squared_soft_posterior_restatement as Q
import squared_soft_restatement as RS


@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_fp64_reproduces_the_enumeration_on_the_tiny_circuits(sum_product):
    plan, tensors, x, cases = Q.tiny_expected(sum_product)
    worst = 0.0
    assert len(cases) == 15
    for s, m, ll, want in cases:
        got, ev = Q.restated_soft_query_log_marginals(plan, tensors, x, ll, RS.mask_of(s, 6), RS.mask_of(m, 6), 3, return_evidence=True)
        assert got.shape == want.shape == (5, len(s), 3)
        inf = torch.isneginf(want)
        assert bool((got[inf] == want[inf]).all()) and bool(inf.any())  # (an exact -inf weight is an exact -inf state)
        worst = max(worst, float((got[~inf] - want[~inf]).abs().max()))
        z = RS.enumerated_soft(plan, tensors, x, ll, RS.mask_of(s, 6), RS.mask_of(m, 6), 3)
        worst = max(worst, float((ev - z).abs().max()), float((torch.logsumexp(got, dim=2) - z[:, None]).abs().max()))
    print(f"{sum_product}: worst fp64 error {worst:.2e}")
    assert worst < 1e-11


@pytest.mark.parametrize("padded", [False, True], ids=["3units", "32units"])
@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_fp32_error_of_the_tiny_circuits(sum_product, padded):
    plan, tensors, x, cases = Q.tiny_expected(sum_product)
    run = R.pad_tiny_to_32(plan, tensors, sum_product) if padded else (plan, tensors)
    for s, m, ll, want in cases:
        got = Q.restated_soft_query_log_marginals(*run, x, ll, RS.mask_of(s, 6), RS.mask_of(m, 6), 3, torch.float32)
        worst, lin, _, _ = P.check(got, want, f"tiny {sum_product} padded={padded} S={s} I={m}", factor=0.5)
        assert worst <= 1.0


@pytest.mark.parametrize("i", range(len(Q.EMB32_SPLITS)))
def test_fp32_error_and_recorded_expectations_of_32_signed_units(i):
    plan, tensors, states = R.emb32_case()
    s, m = Q.EMB32_SPLITS[i]
    rec = Q.golden()[f"emb32_want_{i}"]
    ll = Q.emb32_log_lik(i)
    sm, mm = RS.mask_of(s, 16), RS.mask_of(m, 16)
    assert rec.shape == (33, len(s), 3)
    if len(s) < 16:  # (S = all: 48 fp64 restated passes, recomputed by the recording script alone; the restatement below pins it)
        assert np.allclose(Q.emb32_expected(i), rec, rtol=0, atol=1e-10, equal_nan=True)
    got64 = Q.restated_soft_query_log_marginals(plan, tensors, Q.emb32_rows(), ll, sm, mm, states).numpy()
    fin = np.isfinite(rec)
    assert (got64[~fin] == rec[~fin]).all() and float(np.abs(got64[fin] - rec[fin]).max()) < 1e-9
    got = Q.restated_soft_query_log_marginals(plan, tensors, Q.emb32_rows(), ll, sm, mm, states, torch.float32)
    P.check(got, rec, f"32 signed units S={s} I={m}", factor=0.5)
    for B in (1, 3, 5, 6):  # (the batch sizes the GPU tests slice: the share of states on the linear route holds at each)
        P.check(got[:B], rec[:B], f"32 signed units S={s} I={m} B={B}", factor=0.5)


def test_fp32_error_and_recorded_expectations_of_the_categorical_fixture():
    plan, tensors, states = R.cat_case()
    s, m = Q.CAT_SPLIT
    rec = Q.golden()["cat_want"]
    assert rec.shape == (3, 3, 256)
    fin = np.isfinite(rec)
    want = Q.cat_expected()
    assert (want[~fin] == rec[~fin]).all() and float(np.abs(want[fin] - rec[fin]).max()) < 1e-9
    got = Q.restated_soft_query_log_marginals(plan, tensors, Q.cat_rows(), Q.cat_log_lik(), RS.mask_of(s, 16), RS.mask_of(m, 16), states,
                                              torch.float32)
    # (no signed cancellation in this circuit: every state is held to the bound on its logarithm, as tests/test_squared_down_restatement.py holds it)
    P.check(got, rec, "categorical fixture", factor=0.5, min_log_share=-np.inf)


def test_recorded_draws_and_joint():
    """The first 128 rows of the recorded fp64 sampler (the Philox counter of a row is its index: the rows do not depend on each
    other) and the enumerated joint of the chi-square test; the near rows stay within 2 %."""
    import squared_sampling_restatement as S

    plan, tensors, states = R.emb32_case()
    g = Q.golden()
    x, soft, mask, ll, seed = Q.draw_case()
    out, margin = Q.restated_soft_sampler(plan, tensors, x[:128], ll[:128], soft, mask, states, seed)
    assert np.array_equal(out.numpy(), g["draw_out"][:128]) and np.allclose(margin, g["draw_margin"][:128], rtol=0, atol=1e-9)
    rec = g["draw_out"]
    assert rec.shape == (Q.DRAW_ROWS, 16) and (rec[:, soft] >= 0).all()
    obs = ~(soft | mask)
    assert np.array_equal(rec[:, obs], x.numpy()[:, obs])
    holes = torch.isneginf(ll).numpy()  # no draw outside the support
    assert not holes[np.arange(Q.DRAW_ROWS)[:, None], np.arange(8)[None, :], rec[:, soft]].any()
    assert float(S.near_rows(g["draw_margin"]).mean()) <= 0.02
    assert np.allclose(Q.chi_case()[3], g["chi_joint"], rtol=0, atol=1e-12) and abs(g["chi_joint"].sum() - 1) < 1e-12


@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
def test_the_hand_built_leaf_launches_stay_on_the_logarithm(cplx):
    """The launches the leaf kernel is run on alone (`Q.leaf_case`): only the intended all -inf row and the -inf weights have no
    mass, and at most a quarter of the other states lie below e^-4 of their row's largest (`P.check` of the expectation itself)."""
    for tlog in (False, True):
        for C in (3, 70, 131, 300):
            for K in Q.LEAF_UNITS:
                for B, _ in Q.LEAF_ROWS:
                    _, _, ll, want = Q.leaf_case(cplx, tlog, K, C, B)
                    assert not bool(torch.isnan(want).any())
                    live = want[: B - 1 if B > 1 else B, :2]
                    holes = torch.isneginf(ll[: live.shape[0], :2])
                    for j, Cj in enumerate(Q.leaf_states(C)[:2]):
                        assert bool((torch.isneginf(live[:, j, :Cj]) == holes[:, j, :Cj]).all())
                    P.check(want, want, f"cplx={cplx} tlog={tlog} C={C} K={K} B={B}")


def test_host_plan_under_soft_evidence():
    from cirkit_amd import _capi as capi
    from cirkit_amd.squared_posterior import host_plan
    from cirkit_amd.templates import InputSpec, build_plan, quad_graph

    plan, _, _ = R.emb32_case()
    for s, m in Q.EMB32_SPLITS:
        sm, mm = RS.mask_of(s, 16), RS.mask_of(m, 16)
        dp = host_plan(plan, list(s), mm, soft=sm)
        assert dp.down == P.down_folds(plan, s) and dp.top == P.output_fold(plan) and dp.qvars == sorted(s)
        assert dp.mixed.root[0] == R.MIXED  # (the output fold holds a soft variable: evaluated, its unit 0 is the evidence)
        # every input fold of a soft variable is evaluated, in S order, and its readers see it as a FULL child
        leaves = {(lf.layer, int(f)): int(p) for lf in dp.mixed.leaves for f, p in zip(lf.folds, lf.pos)}
        assert sorted(leaves.values()) == list(range(len(s))) and set(leaves) == set(dp.leaves)
        evaluated = {(la.layer, int(f)) for la in dp.mixed.layers for f in la.folds} | set(leaves)
        assert dp.down <= evaluated  # (the down pass reads the value of every sibling that meets S from the mixed arena)
        where = {(lf.layer, j) for lf in dp.mixed.leaves for j in range(len(lf.folds))}
        read = [int(la.kind[j, h]) for la in dp.mixed.layers for j in range(len(la.folds)) for h in range(la.kind.shape[1])
                if tuple(int(v) for v in la.src[j, h]) in where and int(la.kind[j, h]) == capi.CK_SQ_FULL]
        assert len(read) >= len(s)
        # without `soft` the plan is what the scope sets alone give (`R.classes_from_scopes`, which knows nothing of soft evidence):
        # Q integrated with I, no leaves, exactly the MIXED inner folds evaluated
        plain = host_plan(plan, list(s), sm | mm)
        cls = R.classes_from_scopes(plan, sm | mm)
        assert not plain.mixed.leaves and plain.down == dp.down
        assert all(np.array_equal(a, b) for a, b in zip(plain.mixed.classes, cls))
        assert {(la.layer, int(f)) for la in plain.mixed.layers for f in la.folds} == \
            {(p, f) for p, row in enumerate(cls) for f, c in enumerate(row) if c == R.MIXED and plan.layers[p].inputs is not None}
    dag = build_plan(quad_graph(4, 4), input_layer=InputSpec("embedding", 3), sum_product="cp", num_input_units=2, num_sum_units=2,
                     sum_activation="none", semiring="complex-lse-sum")
    with pytest.raises(NotImplementedError, match="DAG"):
        host_plan(dag, [5, 6], np.zeros(16, dtype=bool), soft=RS.mask_of((5, 6), 16))


def _fake_circuit(plan):
    """What `_Sampler` and the row-byte functions read of a `HipSquaredCircuit`, without a device."""
    from cirkit_amd.squared import HipSquaredCircuit
    from cirkit_amd.squared_graph import FoldGraph

    sq = types.SimpleNamespace(plan=plan, graph=FoldGraph(plan), _const_available=lambda: (lambda p: True), _esize=8, _complex=True,
                               _special=HipSquaredCircuit._special)
    sq._row_bytes = lambda mp: HipSquaredCircuit._row_bytes(sq, mp)
    return sq


def test_row_bytes_hold_the_leaf_blocks_and_the_down_arena():
    from cirkit_amd.squared_posterior import down_row_values, host_plan, row_bytes

    plan, _, _ = R.emb32_case()
    sq = _fake_circuit(plan)
    s, m = Q.EMB32_SPLITS[3]
    dp = host_plan(plan, list(s), RS.mask_of(m, 16), soft=RS.mask_of(s, 16))
    c_row = sum(l.num_folds * l.num_output_units for l in plan.layers)
    mixed = sum(len(la.folds) * sq.graph.units(plan.layers[la.layer]) ** 2 for la in dp.mixed.layers)
    assert down_row_values(sq, dp) == 1024 * (len(dp.down) - 1)
    assert row_bytes(sq, dp) == 8 * (c_row + mixed + 1024 * len(s) + 1024 * (len(dp.down) - 1))


def test_the_sibling_rule_of_sample_soft():
    from cirkit_amd.squared_sampling import MIXED, UNDRAWN, _Sampler

    plan, _, _ = R.emb32_case()
    sm = _Sampler(_fake_circuit(plan))
    none = np.zeros(16, dtype=bool)
    every = np.ones(16, dtype=bool)
    with pytest.raises(NotImplementedError, match=r"variable \d+ is drawn, fold \d+ of layer \d+"):
        sm.order_plan(list(range(16)), none, soft=every)  # raster order: a 2 x 2 block is half drawn when its row ends
    assert not sm.orders  # (nothing was kept)
    order = sm.graph.tree_order()
    op = sm.order_plan(order, none, soft=every)
    assert len(op.steps) == 16 and op.soft_pos == {v: v for v in range(16)}
    seen = set()
    for st in op.steps:
        assert st.mixed is None  # no step needs a soft (or any) re-evaluation
        seen |= {c for row in st.cls for c in row}
        assert MIXED not in seen
    assert UNDRAWN in seen and R.OBSERVED in seen
    # half the pixels soft, one integrated, in tree order: the integrated pixel's siblings take the steps' own mixed launches or constants
    _, soft, mask, _, _ = Q.draw_case()
    op = sm.order_plan([v for v in order if soft[v]], mask, soft=soft)
    assert len(op.steps) == 8 and op.soft_pos == {int(v): j for j, v in enumerate(np.nonzero(soft)[0])}
    # the plans without soft variables are what they were
    a = sm.order_plan(order, none)
    assert all(UNDRAWN not in row for st in a.steps for row in st.cls)


def test_refusals_of_the_sets():
    from cirkit_amd.squared_graph import FoldGraph
    from cirkit_amd.squared_soft import check_sets

    plan, _, _ = R.emb32_case()
    g = FoldGraph(plan)
    none = np.zeros(16, dtype=bool)
    with pytest.raises(ValueError, match="at least one"):
        check_sets(g, none, none, "soft evidence")
    with pytest.raises(ValueError, match="both soft and integrated"):
        check_sets(g, RS.mask_of((1, 2), 16), RS.mask_of((2,), 16), "soft evidence")
    gplan, _, _ = R.gauss_case()
    with pytest.raises(NotImplementedError, match="Gaussian"):
        check_sets(FoldGraph(gplan), RS.mask_of((0,), gplan.num_variables), np.zeros(gplan.num_variables, dtype=bool), "soft evidence")
