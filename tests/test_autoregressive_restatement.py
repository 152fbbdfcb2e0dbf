"""The numpy restatement of the autoregressive conditionals (tests/autoregressive_restatement.py; DESIGN.md section 11,
"Autoregressive conditionals and coding") pinned on the CPU: against brute force by enumeration on the oracle, by the chain
rule against the fp64 log p(x), and the numpy quantiser by its properties.  The refusals of
`HipCircuit.autoregressive_conditionals` / `coding_tables` that need no device are here too."""
import numpy as np
import pytest

from autoregressive_restatement import (autoregressive_restated, brute_force, covered, expand, log_prob_restated, quantise)
from test_loo_restatement import KAT, any_case
from test_mpe import _case
from test_posterior_marginals import _exact, _states

NEW_ENTRY_POINTS = ("ck_ar_expand", "ck_ar_leaf_categorical", "ck_ar_leaf_gaussian", "ck_ar_log_probs", "ck_ar_quantise")
CHAIN_PLANS = ["kat_bernoulli_f0o0", "kat_bernoulli_f1o1", "quadtree_4x4_kron_k3", "plan_quadgraph_1x4x4_cp",
               "quadgraph_6x6_tucker_k4", "binomial_qg6x6_k4", "pd_gauss_6x6_k4", "plan_clt_mixed6_cp", "qt2_cp_k32"]


def evidence(plan, B, seed) -> np.ndarray:
    rng = np.random.default_rng(seed)
    c = _states(plan)
    x = rng.normal(size=(B, plan.num_variables))
    d = c > 0
    x[:, d] = rng.integers(0, c[d], size=(B, int(d.sum())))
    return x


# ------------------------------------------------------------------------------------------------------------ brute force
@pytest.mark.parametrize("order_kind", ["ascending", "reversed", "permuted"])
@pytest.mark.parametrize("name", KAT)
def test_restatement_is_brute_force_on_the_oracle(name, order_kind):
    plan, tensors = _exact(*_case(name))
    D = plan.num_variables
    order = {"ascending": None, "reversed": list(range(D))[::-1],
             "permuted": [int(v) for v in np.random.default_rng(41).permutation(D)]}[order_kind]
    x = evidence(plan, 12, 42)
    res = autoregressive_restated(plan, tensors, x, order)
    p, logp = brute_force(plan, tensors, x, order)
    assert res["p"].shape == p.shape and np.isfinite(res["p"]).all()
    assert np.abs(res["p"] - p).max() <= 1e-12
    assert np.abs(res["logp"] - logp).max() <= 1e-12
    sub = autoregressive_restated(plan, tensors, x, order, [1, D - 1])
    assert np.array_equal(sub["p"], res["p"][:, [1, D - 1]]) and np.array_equal(sub["logp"], res["logp"][:, [1, D - 1]])


def test_expansion_hides_the_steps_from_the_position_on():
    plan, _ = _case("kat_bernoulli_f1o1")
    D = plan.num_variables
    x = evidence(plan, 2, 43)
    x[1, 2] = -1  # a sentinel of the caller's stays missing at every step
    order = [3, 0, 4, 1, 2][:D]
    xe, mask, _, pos = expand(plan, x, order, [0, 2])
    assert xe.shape == (4, D) and pos == [0, 2]
    assert mask[0].all() and mask[2, [0, 1, 3, 4]].all() and mask[2, 2]
    assert mask[1].tolist() == [v in (4, 1, 2) for v in range(D)]
    assert mask[3].tolist() == [v in (4, 1, 2) for v in range(D)]
    _, keep, _, _ = expand(plan, x, order, [0, 2], keep_own=True)
    assert keep[1].tolist() == [v in (1, 2) for v in range(D)]


# ------------------------------------------------------------------------------------------------------------- chain rule
@pytest.mark.parametrize("name", CHAIN_PLANS)
def test_chain_rule_sums_to_the_log_probability(name):
    plan, tensors = any_case(name)
    x = evidence(plan, 3, 44)
    order = [int(v) for v in np.random.default_rng(45).permutation(covered(plan))]
    want = log_prob_restated(plan, tensors, x)
    for o in (None, order):
        res = autoregressive_restated(plan, tensors, x, o)
        assert np.isfinite(res["logp"]).all()
        # fp64, len(order) terms, each a difference of two log-sum-exps of the size of log c(x)
        assert np.abs(res["logp"].sum(1) - want).max() <= 1e-9 * (1 + np.abs(want).max())
        if res["p"] is not None and _states(plan).max() > 0:
            assert np.abs(res["p"].sum(2) - 1).max() <= 1e-12
            got = np.take_along_axis(res["p"], x[:, res["order"]].astype(np.int64)[:, :, None], axis=2)[:, :, 0]
            assert np.abs(np.log(got) - res["logp"]).max() <= 1e-9


def test_a_missing_step_reads_zero_and_stays_missing():
    plan, tensors = any_case("quadtree_4x4_kron_k3")
    x = evidence(plan, 2, 46)
    x[0, 5] = -1
    res = autoregressive_restated(plan, tensors, x)
    assert res["logp"][0, 5] == 0 and res["missing"][0, 5] and not res["missing"][1].any()
    assert np.abs(res["p"][0, 5].sum() - 1) <= 1e-12  # (the conditional of a missing variable is still its posterior)
    # the later steps of row 0 are those of the row without variable 5: its chain sums to the marginal of the rest
    from loo_restatement import leave_one_out_restated

    rest = leave_one_out_restated(plan, tensors, x[:1], [0], [5])["logev"][0]
    z = leave_one_out_restated(plan, tensors, x[:1], [0], np.ones(plan.num_variables, dtype=bool))["logev"][0]
    assert abs(res["logp"][0].sum() - (rest - z)) <= 1e-9


# -------------------------------------------------------------------------------------------------------------- quantiser
def adversarial_rows():
    """(p (rows, 256) fp32, nstates (rows,)): one state with all the mass, all states equal, fp32 row sums of 1 +- 2e-5, a NaN
    row, a row over fewer states than the table is wide."""
    rng = np.random.default_rng(47)
    C = 256
    rows, ns = [], []
    one = np.zeros(C, dtype=np.float32)
    one[77] = 1.0
    rows.append(one)
    ns.append(C)
    rows.append(np.full(C, 1.0 / C, dtype=np.float32))
    ns.append(C)
    for scale in (1 + 2e-5, 1 - 2e-5):
        r = rng.dirichlet(np.full(C, 0.3)).astype(np.float32)
        rows.append((r * np.float32(scale / r.astype(np.float64).sum())).astype(np.float32))
        ns.append(C)
    bad = rng.dirichlet(np.ones(C)).astype(np.float32)
    bad[3] = np.nan
    rows.append(bad)
    ns.append(C)
    few = np.zeros(C, dtype=np.float32)
    few[:5] = rng.dirichlet(np.ones(5)).astype(np.float32)
    rows.append(few)
    ns.append(5)
    tie = np.zeros(C, dtype=np.float32)
    tie[[9, 200]] = 0.5  # two largest counts: the slack goes to the first
    rows.append(tie)
    ns.append(C)
    return np.stack(rows), np.asarray(ns)


def check_tables(t, p, ns, precision):
    T, C = 1 << precision, p.shape[1]
    cnt = np.diff(t.astype(np.int64), axis=1)
    assert t.dtype == np.int32 and t.shape == (p.shape[0], C + 1)
    assert (t[:, 0] == 0).all() and (t[:, -1] == T).all()
    live = np.arange(C)[None] < ns[:, None]
    assert (cnt[live] >= 1).all() and (cnt[~live] == 0).all()
    nan = np.isnan(p).any(axis=1)
    for r in np.nonzero(nan)[0]:
        assert cnt[r, : ns[r]].max() - cnt[r, : ns[r]].min() <= T % ns[r] and cnt[r, 1 : ns[r]].max() == T // ns[r]
    return cnt


@pytest.mark.parametrize("precision", [10, 12, 16, 24])
def test_quantiser_meets_its_properties(precision):
    p, ns = adversarial_rows()  # C = 256 at precision 10 is the refusal boundary
    cnt = check_tables(quantise(p, ns, precision), p, ns, precision)
    T = 1 << precision
    assert cnt[0, 77] == T - 255 and cnt[1].min() >= T // 256 - 1
    assert cnt[6, 9] >= cnt[6, 200]  # (the first of two equal largest counts takes the slack)
    rng = np.random.default_rng(48)
    for C, S in ((2, 2), (3, 2), (17, 17), (64, 33), (256, 256)):
        if C > 2 ** (precision - 2):
            continue
        q = np.zeros((40, C), dtype=np.float32)
        q[:, :S] = rng.dirichlet(np.full(S, 0.5), size=40).astype(np.float32)
        ns = np.full(40, S)
        cnt = check_tables(quantise(q, ns, precision), q, ns, precision)
        # close to the distribution: no state is off by more than the floor and the slack
        assert np.abs(cnt / T - q).max() <= (2.0 * S + 2) / T + 1e-6


def test_quantiser_is_a_function_of_the_fp32_vector_alone():
    p, ns = adversarial_rows()
    a = quantise(p, ns, 16)
    b = quantise(p.astype(np.float64), ns, 16)  # (fp64 input is rounded to fp32 first)
    assert np.array_equal(a, b) and np.array_equal(a, quantise(p[::-1], ns[::-1], 16)[::-1])


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_need_no_device():
    from cirkit_amd.autoregressive import check_order, check_positions, check_precision, state_counts
    from cirkit_amd.topdown import variable_kinds

    plan = _case("cfg1_rbt8")[0]
    D, kinds = plan.num_variables, variable_kinds(plan)
    assert check_order(kinds, D, None) == list(range(D))
    assert check_order(kinds, D, list(range(D))[::-1]) == list(range(D))[::-1]
    assert check_order(kinds, D, np.arange(D)) == list(range(D))
    with pytest.raises(ValueError, match="more than once"):
        check_order(kinds, D, [0] + list(range(D - 1)))
    with pytest.raises(ValueError, match="outside 0"):
        check_order(kinds, D, list(range(1, D + 1)))
    with pytest.raises(ValueError, match="left out"):
        check_order(kinds, D, list(range(D - 1)))
    part = {v: k for v, k in kinds.items() if v != 2}
    with pytest.raises(ValueError, match="scope of every input layer"):
        check_order(part, D, list(range(D)))
    assert check_positions(5, None) == [0, 1, 2, 3, 4]
    assert check_positions(5, [4, 1, 1]) == [1, 4] and check_positions(5, range(2, 4)) == [2, 3]
    import torch

    assert check_positions(5, torch.tensor([True, False, False, True, False])) == [0, 3]
    with pytest.raises(ValueError):
        check_positions(5, [5])
    with pytest.raises(ValueError):
        check_positions(5, [-1])
    with pytest.raises(ValueError):
        check_positions(5, [])
    with pytest.raises(ValueError):
        check_positions(5, torch.zeros(4, dtype=torch.bool))
    for bad in (7, 25, 16.5):
        with pytest.raises(ValueError):
            check_precision(bad, 2)
    with pytest.raises(ValueError, match="states"):
        check_precision(10, 257)
    assert check_precision(10, 256) == 10 and check_precision(8, 64) == 8 and check_precision(24, 256) == 24
    assert state_counts(plan).tolist() == _states(plan).tolist()
    mixed = _case("plan_clt_mixed6_cp")[0]
    assert state_counts(mixed).tolist() == _states(mixed).tolist()


def test_autoregressive_entry_points_are_exported_at_abi_51():
    from cirkit_amd import _capi as capi

    lib = capi.load()
    assert lib.ck_abi_version() == 51
    for n in NEW_ENTRY_POINTS:
        assert hasattr(lib, n) and n in capi.SIGNATURES
    assert lib.ck_ar_quantise(None, None, None, 1, 1, 16, None, None) == -1
    assert b"ck_ar_quantise" in lib.ck_last_error()
