"""The algorithm of sampling squared circuits (cirkit_amd/squared_sampling.py) against fp64 enumeration, on the host: the
restatement (tests/squared_sampling_restatement.py) of the path gradient and the leaf form in fp64 reproduces
``logsumexp(2 Re log c)`` over the completions for EVERY state of a variable; in fp32 it stays below a quarter of the bound the
GPU tests assert (``1e-4 max(1, |want|)``, `R.bound`); the restated sampler draws the exact distribution; the depth-first order
never meets a mixed sibling; a DAG is refused; and the near-boundary tolerance of the draw-for-draw GPU tests is measured here.

Measured (printed by the tests): worst fp64 error 1.7e-12; worst fp32 error as a fraction of the bound: tiny cp-t 0.006, tiny
cp 0.106 (padded to 32 units 0.005 and 0.224), 32 signed units 0.107, the Categorical fixture 0.001; worst |CDF_fp32 - CDF_fp64|
2.8e-5 / 3.1e-5 / 2.2e-5 (default order, raster order, half the pixels observed; EPS = 4e-5 asserted), rows flagged near by the
fp64 run 0.83 % / 1.27 % / 0.49 % (2 % allowed); the hand-built paths of the kernel-alone test 0.002 of the bound.

Running time: about 105 s on 8 cores, which is what recomputing the recorded expectations costs -- 75 s for the three restated
samplers on 2048 rows x 16 steps in fp64 and fp32 (`test_near_boundary_tolerance_of_the_draw_for_draw_cases`), 15 s for the
enumerations of the 32-unit and Categorical cases, 10 s for the two chi-square runs of 2^18 host draws; everything else is
below a second."""
import numpy as np
import pytest
import torch

import squared_marginal_restatement as R
import squared_sampling_restatement as S
from cirkit_amd.squared_sampling import path_plan, scope_bits, tree_order


def _frac(got, want):
    got, want = got.double(), want.double()
    fin = torch.isfinite(want)
    assert bool((got[~fin] == want[~fin]).all())
    return float(((got[fin] - want[fin]).abs() / torch.from_numpy(R.bound(want[fin]))).max()) if bool(fin.any()) else 0.0


@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_every_variable_and_mask_of_the_tiny_circuits(sum_product):
    """All 6 variables, all 32 masks of the other five, 5 rows, all 3 states: fp64 to rounding."""
    plan, tensors, states = R.tiny_case(sum_product)
    x = R.rows_of(6, states, 5)
    worst = 0.0
    for v in range(6):
        others = [w for w in range(6) if w != v]
        for j in range(32):
            mask = np.zeros(6, dtype=bool)
            mask[[w for k, w in enumerate(others) if (j >> k) & 1]] = True
            want = S.enumerated_state_log_marginals(plan, tensors, x, v, mask, states)
            got = S.restated_state_log_marginals(plan, tensors, x, v, mask, states)
            worst = max(worst, float((got - want).abs().max()))
    print(f"{sum_product}: worst fp64 error {worst:.2e}")
    assert worst < 1e-11


@pytest.mark.parametrize("padded", [False, True], ids=["3units", "32units"])
@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_fp32_error_of_the_tiny_queries(sum_product, padded):
    plan, tensors, states = R.tiny_case(sum_product)
    x = R.rows_of(6, states, 5, seed=S.TINY_ROWS_SEED)
    run = R.pad_tiny_to_32(plan, tensors, sum_product) if padded else (plan, tensors)
    worst = 0.0
    for v, mask in S.tiny_queries():
        want = S.enumerated_state_log_marginals(plan, tensors, x, v, mask, states)
        if padded:
            assert float((S.restated_state_log_marginals(*run, x, v, mask, states) - want).abs().max()) < 1e-11
        worst = max(worst, _frac(S.restated_state_log_marginals(*run, x, v, mask, states, torch.float32), want))
    print(f"tiny {sum_product} padded={padded}: worst fp32 error {worst:.3f} of the bound")
    assert worst < 0.25


def test_fp32_error_of_32_signed_units():
    """The recorded rows and expectations are what the enumeration gives; every state holds at least e^-4 of its row's
    largest (`S.emb32_rows_and_expected` says why); fp64 to rounding, fp32 below a quarter of the bound."""
    plan, tensors, states = R.emb32_case()
    g = S.golden()
    x = torch.from_numpy(g["emb32_x"])
    assert x.shape == (33, 16)
    pool = R.rows_of(16, states, *S.EMB32_POOL)
    assert all(bool((pool == r).all(dim=1).any()) for r in x)  # (rows of the pool)
    worst = 0.0
    for (v, mask), rec in zip(S.emb32_queries(), g["emb32_want"]):
        want = S.enumerated_state_log_marginals(plan, tensors, x, v, mask, states)
        assert np.allclose(want.numpy(), rec, rtol=0, atol=1e-10)
        assert float(S.log_share(rec).min()) >= S.MIN_LOG_SHARE
        assert float((S.restated_state_log_marginals(plan, tensors, x, v, mask, states) - want).abs().max()) < 1e-10
        worst = max(worst, _frac(S.restated_state_log_marginals(plan, tensors, x, v, mask, states, torch.float32), want))
    print(f"32 signed units: worst fp32 error {worst:.3f} of the bound")
    assert worst < 0.25


def test_fp32_error_of_the_categorical_fixture():
    plan, tensors, states = R.cat_case()
    x = torch.from_numpy(np.random.default_rng(S.CAT_ROWS_SEED).integers(0, states, size=(3, 16)))
    worst = 0.0
    for (v, mask), rec in zip(S.cat_queries(), S.golden()["cat_want"]):
        want = S.enumerated_state_log_marginals(plan, tensors, x, v, mask, states)
        assert np.allclose(want.numpy(), rec, rtol=0, atol=1e-10)
        if int(mask.sum()) <= 1:  # (enumerated: the fp64 restatement is pinned to it)
            assert float((S.restated_state_log_marginals(plan, tensors, x, v, mask, states) - want).abs().max()) < 1e-10
        worst = max(worst, _frac(S.restated_state_log_marginals(plan, tensors, x, v, mask, states, torch.float32), want))
    print(f"categorical fixture: worst fp32 error {worst:.3f} of the bound")
    assert worst < 0.25


@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
def test_fp32_error_of_the_hand_built_paths(cplx):
    """The paths the kernel is run on alone (`S.hand_path_case`): only the intended all -inf row has no mass, every other state
    holds at least e^-4 of its row's largest, and the fp32 restatement of the path stays below a quarter of the bound."""
    worst = 0.0
    for shape in S.PATH_SHAPES:
        for B in (1, 3):
            case, want, want32, _ = S.hand_path_case(cplx, shape, B)
            live = torch.isfinite(want).any(dim=1)
            rank1 = any(kd == S.KIND_RANK1 for lv in case[0] for kd, _, _ in lv[4])
            assert want.shape == (B, S.PATH_STATES) and int((~live).sum()) == (1 if B > 1 and rank1 else 0)
            assert float(S.log_share(want[live].numpy()).min()) >= S.MIN_LOG_SHARE
            worst = max(worst, _frac(want32, want))
    print(f"hand-built paths: worst fp32 error {worst:.4f} of the bound")
    assert worst < 0.25


@pytest.mark.parametrize("side", [4, 8])
def test_tree_order_meets_no_mixed_sibling(side):
    from cirkit_amd.templates import InputSpec, build_plan, quad_tree

    plan = build_plan(quad_tree(side, side), input_layer=InputSpec("embedding", 3), sum_product="cp", num_input_units=2,
                      num_sum_units=2, sum_activation="none", semiring="complex-lse-sum")
    D = side * side
    order = tree_order(plan)
    assert sorted(order) == list(range(D))
    bits = scope_bits(plan)
    scopes = R.fold_scopes(plan)
    assert all(bits[i][f] == sum(1 << v for v in s) for i, layer in enumerate(scopes) for f, s in enumerate(layer))
    for i, v in enumerate(order):
        mask = np.zeros(D, dtype=bool)
        mask[order[i:]] = True  # v and everything after it
        cls = R.classes_from_scopes(plan, mask)
        pp = path_plan(plan, v)
        assert len(pp.levels) > 0 and plan.layers[pp.leaf[0]].inputs is None
        for lv in pp.levels:
            assert all(cls[p][g] != R.MIXED for p, g in lv.siblings), (v, lv)
    raster = list(range(D))  # (another order does meet them)
    met = False
    for i, v in enumerate(raster):
        mask = np.zeros(D, dtype=bool)
        mask[raster[i:]] = True
        cls = R.classes_from_scopes(plan, mask)
        met = met or any(cls[p][g] == R.MIXED for lv in path_plan(plan, v).levels for p, g in lv.siblings)
    assert met


def test_a_dag_is_refused():
    from cirkit_amd.templates import InputSpec, build_plan, quad_graph

    plan = build_plan(quad_graph(4, 4), input_layer=InputSpec("embedding", 3), sum_product="cp", num_input_units=2,
                      num_sum_units=2, sum_activation="none", semiring="complex-lse-sum")
    with pytest.raises(NotImplementedError, match="DAG"):
        for v in range(16):
            path_plan(plan, v)


def _chi2_p(counts, expected):
    """tests/test_sampling.py::_chi2_p: cells with tiny expectations merged into one."""
    scipy_stats = pytest.importorskip("scipy.stats")
    keep = expected >= 5
    obs = np.append(counts[keep], counts[~keep].sum())
    exp = np.append(expected[keep], expected[~keep].sum())
    if exp[-1] == 0:
        obs, exp = obs[:-1], exp[:-1]
    exp = exp * obs.sum() / exp.sum()
    return float(scipy_stats.chisquare(obs, exp).pvalue)


@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_the_restated_sampler_is_exact(sum_product):
    pytest.importorskip("scipy.stats")
    plan, tensors, states = R.tiny_case(sum_product)
    N = 1 << 18
    out, _, _ = S.restated_sampler(plan, tensors, torch.zeros((N, 6), dtype=torch.int64), np.ones(6, dtype=bool), states, seed=20250104)
    assert int(out.min()) >= 0
    worlds = R.all_worlds(6, states)
    p = torch.softmax(R.log_c2_of(plan, tensors, worlds), dim=0).numpy()
    counts = np.bincount(S.world_codes(out.numpy(), states), minlength=states ** 6)
    assert _chi2_p(counts, p * N) >= 1e-6


@pytest.mark.parametrize("name", ["default", "raster", "conditional"])
def test_near_boundary_tolerance_of_the_draw_for_draw_cases(name):
    """The fp32-restated normalised CDF stays within EPS of the fp64 one at every step, the fp64 run alone flags at most 2 % of
    the rows near (within 4 EPS of a boundary of the chosen bin), and the recorded draws are the fp64 run's."""
    x, drawn, order, seed = S.draw_cases()[name]
    out, margin, worst = S.draw_expected(name, compare=torch.float32)
    near = S.near_rows(margin)
    print(f"{name}: worst |CDF32 - CDF64| {worst:.2e} (EPS {S.EPS:.0e}), near rows {100 * float(near.mean()):.2f} %")
    assert worst <= S.EPS
    assert float(near.mean()) <= 0.02
    keep = ~torch.from_numpy(drawn)
    assert int(out.min()) >= 0 and bool((torch.from_numpy(out.astype(np.int64))[:, keep] == x[:, keep]).all())
    g = S.golden()
    assert np.array_equal(g[f"draw_{name}_out"][~near], out[~near])
    assert np.array_equal(S.near_rows(g[f"draw_{name}_margin"]), near) or float(np.abs(g[f"draw_{name}_margin"] - margin).max()) < 1e-9
