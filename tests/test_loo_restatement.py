"""The numpy restatement of the leave-one-out conditionals (tests/loo_restatement.py; DESIGN.md section 11, "Leave-one-out
conditionals") pinned on the CPU: against brute force on the oracle, against the posterior restatement with the variable
added to the missing set (the defining identity), by the conservation identity lse_k(D_k + v_k) = log c(x_O), and on tables
with exact zeros, where the flow-form shortcut f_k / u_k is wrong.  The refusals of `HipCircuit.leave_one_out` that need no
device are here too."""
import functools
import types

import numpy as np
import pytest
import torch

from loo_restatement import leave_one_out_restated
from posterior_restatement import posterior_restated
from test_em_restatement import TEMPLATES, _any
from test_expected_statistics import SMALL, _random_x, _small
from test_mpe import PLANS, _case
from test_posterior_marginals import _exact, _states

KAT = ["kat_bernoulli_f0o0", "kat_bernoulli_f0o1", "kat_bernoulli_f1o0", "kat_bernoulli_f1o1"]
IDENTITY_PLANS = list(SMALL) + list(TEMPLATES) + [p for p in PLANS if p not in ("cfg2_qt784", "cfg4_pd784")]
NEW_ENTRY_POINTS = ("ck_loo_down_sum", "ck_loo_segment_lse", "ck_loo_down_product", "ck_loo_leaf_categorical",
                    "ck_loo_leaf_gaussian", "ck_loo_log_probs")


def any_case(name):
    """(plan, tensors) of a SMALL, TEMPLATES or fixture plan, bare `probs` normalised in fp64 (`_exact` says why)."""
    return _exact(*(_small(name) if name in SMALL else _any(name)))


def brute_force(plan, tensors, x, mask):
    """(joint (B, D, C) log p(X_v = c, x_{O \\ v}) with -inf past a variable's states, by one oracle marginal forward per
    (variable, state)) for a discrete plan; `mask` (B, D) marks what every row misses."""
    from oracle.torch_oracle import as_torch, evaluate_plan

    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # (the oracle's Binomial: tests/test_posterior_marginals.py explains)
    try:
        tt = {k: v.double() for k, v in as_torch(tensors).items()}
        B, D = x.shape
        states = _states(plan)
        joint = np.full((B, D, int(states.max())), -np.inf)
        for v in range(D):
            m = torch.from_numpy(mask.copy())
            m[:, v] = False
            for c in range(int(states[v])):
                xs = torch.from_numpy(np.where(mask, 0, x).astype(np.int64))
                xs[:, v] = c
                joint[:, v, c] = evaluate_plan(plan, tt, xs, integrate_mask=m)[:, 0, 0].numpy()
    finally:
        torch.set_default_dtype(default)
    return joint


def normalised(joint):
    """exp(joint) over its sum over the states; NaN where there is no mass."""
    mx = joint.max(axis=2, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.exp(joint - np.where(np.isfinite(mx), mx, 0))
        tot = e.sum(axis=2, keepdims=True)
        return np.where(tot > 0, e / np.where(tot > 0, tot, 1), np.nan)


def _same(a, b, tol):
    """Equal within tol, NaN and infinities in the same places."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    return bool(((a == b) | (np.isnan(a) & np.isnan(b)) | fin).all()) and (not fin.any() or float(np.abs(a[fin] - b[fin]).max()) <= tol)


# ------------------------------------------------------------------------------------------------------------ brute force
@pytest.mark.parametrize("name", KAT)
def test_restatement_is_brute_force_on_the_oracle(name):
    plan, tensors = _exact(*_case(name))
    D, B = plan.num_variables, 48
    rng = np.random.default_rng(21)
    x = _random_x(plan, B, rng)
    mask = rng.random((B, D)) < 0.3
    mask[0] = False
    res = leave_one_out_restated(plan, tensors, x, list(range(D)), mask)
    joint = brute_force(plan, tensors, x, mask)
    want = normalised(joint)
    assert np.isfinite(res["p"]).all() and np.abs(res["p"] - want).max() <= 1e-10
    obs = np.take_along_axis(joint, x.astype(np.int64)[:, :, None], axis=2)[:, :, 0]
    mx = joint.max(axis=2)
    lse = mx + np.log(np.exp(joint - mx[:, :, None]).sum(axis=2))
    assert np.abs(res["logp"] - np.where(mask, 0, obs - lse)).max() <= 1e-10
    assert (res["logp"][mask] == 0).all()


# ---------------------------------------------------------------------------------------- the defining identity, conservation
@pytest.mark.parametrize("name", IDENTITY_PLANS)
def test_leave_one_out_is_the_posterior_with_the_variable_missing(name):
    plan, tensors = any_case(name)
    D, B = plan.num_variables, 6
    rng = np.random.default_rng(22)
    x = _random_x(plan, B, rng)
    miss = np.nonzero(rng.random(D) < 0.25)[0]
    gauss = any(l.type == "gaussian" for l in plan.layers)
    xm = x.copy()
    xm[:, miss] = np.nan if gauss else -1
    res = leave_one_out_restated(plan, tensors, x, list(range(D)), miss)
    assert np.isfinite(res["p"]).all() and np.isfinite(res["logev"]).all()
    # conservation: multilinearity gives lse_k(D_k + v_k) = log c(x_O) for every variable
    assert np.abs(res["cons"] - res["logev"][:, None]).max() <= 1e-10 * (1 + np.abs(res["logev"]).max())
    if not gauss:
        assert np.abs(res["p"].sum(2) - 1).max() <= 1e-12
    for q, v in enumerate(res["query"]):
        post = posterior_restated(plan, tensors, xm, [v])["p"][:, 0]
        got = res["p"][:, q, : post.shape[1]]
        err = np.abs(got - post) / (1 + np.abs(post)) if gauss else np.abs(got - post)
        assert err.max() <= 1e-10, (v, err.max())
        assert (res["p"][:, q, post.shape[1] :] == 0).all()


LIST_PLANS = ("plan_quadgraph_1x4x4_cp", "quadgraph_6x6_tucker_k4", "quadtree_4x4_kron_k3", "pd_gauss_6x6_k4")


def test_message_lists_follow_the_consumer_lists():
    from cirkit_amd.leave_one_out import message_lists
    from cirkit_amd.posterior import consumer_lists

    for name in ("plan_quadgraph_1x4x4_cp", "quadgraph_6x6_tucker_k4", "quadtree_4x4_kron_k3", "pd_gauss_6x6_k4"):
        plan = _case(name)[0]
        for a, b in zip(message_lists(plan), consumer_lists(plan)):
            assert (a is None) == (b is None)
            if a is not None:
                for n in ("children", "start", "first"):
                    assert np.array_equal(a[n], b[n]), (name, n)


@pytest.mark.parametrize("per_input", [False, True])
def test_consumer_lists_hold_every_pair_once(per_input):
    """The one list builder (cirkit_amd/topdown.py), both modes: every (consumer fold, input position) pair is decoded from
    `items` exactly once across the layers, under the child it feeds; `first` is set on exactly the last-walked layer that
    feeds each child; `slots` is the number of distinct message slots."""
    from cirkit_amd.plan import resolve_fold_index
    from cirkit_amd.topdown import consumer_lists

    for name in LIST_PLANS:
        plan = _case(name)[0]
        folds = [l.num_folds for l in plan.layers]
        off = np.concatenate([[0], np.cumsum(folds)])
        lists = consumer_lists(plan, per_input)
        assert len(lists) == len(plan.layers)
        want, got = {}, {}  # (consumer global fold, input position) -> child global fold
        firsts: dict[int, list[int]] = {}  # child global fold -> the layers marked `first` for it
        feeders: dict[int, list[int]] = {}  # child global fold -> the layers that feed it
        for j, (l, c) in enumerate(zip(plan.layers, lists)):
            assert (c is None) == (l.inputs is None), (name, j)
            if c is None:
                continue
            H, F = l.arity, l.num_folds
            ch = resolve_fold_index(l.inputs, folds)
            for f in range(F):
                for h in range(H):
                    want[(int(off[j]) + f, h)] = int(off[ch[f, h, 0]] + ch[f, h, 1])
            children, start = c["children"].tolist(), c["start"].tolist()
            assert children == sorted(set(children)) and start[0] == 0 and len(start) == len(children) + 1
            pairs = l.type == "kronecker" or (l.type == "hadamard" and per_input)
            items = c["items"].reshape(-1, 2).tolist() if pairs else c["items"].tolist()
            assert start[-1] == len(items) == F * H, (name, j)
            slots = set()
            for k, child in enumerate(children):
                feeders.setdefault(child, []).append(j)
                if c["first"][k]:
                    firsts.setdefault(child, []).append(j)
                for it in items[start[k] : start[k + 1]]:
                    if pairs:
                        decoded = [(it[0], it[1])]
                    elif l.type == "hadamard":  # one item per consumer fold and input position, all naming the fold
                        decoded = [(it, h) for h in range(H) if want[(it, h)] == child and (it, h) not in got][:1]
                    elif l.type == "cpt" and not per_input:  # slot f, shared by the fold's inputs
                        slots.add(it)
                        decoded = [(int(off[j]) + it, h) for h in range(H) if want[(int(off[j]) + it, h)] == child
                                   and (int(off[j]) + it, h) not in got][:1]
                    else:  # slot f H + h
                        slots.add(it)
                        decoded = [(int(off[j]) + it // H, it % H)]
                    assert len(decoded) == 1 and decoded[0] not in got, (name, j, it)
                    got[decoded[0]] = child
            assert c["slots"] == len(slots), (name, j)
        assert got == want, name
        for child, js in feeders.items():  # the pass walks the layers last to first: the first writer is the LAST layer
            assert firsts.get(child) == [max(js)], (name, child)


# ------------------------------------------------------------------------------------------------------------------ zeros
@functools.lru_cache(maxsize=None)
def zero_case():
    """kat_bernoulli_f1o1 (bare `probs`, two units per variable) with exact zeros: both units of variable 0 call state 1
    impossible, unit 0 of variable 1 calls state 1 impossible.  Rows: 0 observes x_1 = 1 (unit 0 of variable 1 has value
    -inf and still carries leave-one-out mass), 1 observes x_0 = 1 (c(x_O) = 0, the conditional of variable 0 exists, the
    others' do not), 2 both, the rest random with x_0 = 0.  Returns (plan, tensors, x, name of the table tensor)."""
    plan, tensors = _case("kat_bernoulli_f1o1")
    cat = plan.layers[0]
    name = cat.params["probs"].nodes[0].config["tensor"]
    assert cat.scope_idx[:2, 0].tolist() == [0, 1]
    t = np.asarray(tensors[name], dtype=np.float64).copy()
    t[0, :, 1] = 0.0
    t[1, 0, 1] = 0.0
    t /= t.sum(axis=-1, keepdims=True)
    tensors = dict(tensors)
    tensors[name] = t.astype(np.float32)
    rng = np.random.default_rng(23)
    x = rng.integers(0, 2, size=(12, plan.num_variables)).astype(np.float64)
    x[:, 0] = 0
    x[0, :2] = (0, 1)
    x[1, :2] = (1, 0)
    x[2, :2] = (1, 1)
    return plan, tensors, x, name


def test_zeros_match_brute_force_where_the_flow_form_does_not():
    plan, tensors, x, _ = zero_case()
    plan, tensors = _exact(plan, tensors)
    B, D = x.shape
    mask = np.zeros((B, D), dtype=bool)
    res = leave_one_out_restated(plan, tensors, x, list(range(D)))
    joint = brute_force(plan, tensors, x, mask)
    want = normalised(joint)
    assert _same(res["p"], want, 1e-10)
    # the case is not vacuous: units that give the OBSERVED state probability 0 carry a real share of the mass
    assert res["zero_share"][0, 1] > 0.1 and res["zero_share"][1, 0] > 0.1
    # a row without mass whose leave-one-out distribution exists, and is the point mass; its other variables have none
    assert res["logev"][1] == -np.inf and np.array_equal(res["p"][1, 0], [1.0, 0.0])
    assert np.isnan(res["p"][1, 1:]).all() and np.isnan(res["logp"][1, 1:]).all() and res["logp"][1, 0] == -np.inf
    obs = np.take_along_axis(joint, x.astype(np.int64)[:, :, None], axis=2)[:, :, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        lp = obs - np.log(np.exp(joint).sum(axis=2))
    assert _same(res["logp"], lp, 1e-10)
    # the flow form f_k / u_k = exp(D_k) where u_k > 0, nothing where u_k = 0: wrong in row 0, 0 / 0 in row 1
    short = np.empty_like(want)
    for v, (Dc, vc, lz, nt) in res["units"].items():
        with np.errstate(invalid="ignore", divide="ignore"):
            a = (np.where(vc > -np.inf, np.exp(Dc + lz[None]), 0)) @ nt
            short[:, v] = a / a.sum(axis=1, keepdims=True)
    assert np.abs(short[0, 1] - want[0, 1]).max() > 0.05
    assert np.isnan(short[1, 0]).all() and np.isfinite(want[1, 0]).all()


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_need_no_device():
    from cirkit_amd.leave_one_out import LeaveOneOutQuery, check_query_vars, variable_kinds

    squared = _case("cfg5_sos_c_k32")[0]
    with pytest.raises(ValueError, match="lse-sum"):
        LeaveOneOutQuery(types.SimpleNamespace(user_plan=squared))
    import copy

    plan = _case("cfg1_rbt8")[0]
    for kind, cls in (("embedding", "TorchEmbeddingLayer"), ("constant", "TorchConstantValueLayer"),
                      ("tensordot", "TorchTensorDotLayer")):
        bad = copy.deepcopy(plan)
        bad.layers[1].type = kind
        with pytest.raises(TypeError, match=cls):
            LeaveOneOutQuery(types.SimpleNamespace(user_plan=bad))
    D = plan.num_variables
    kinds = variable_kinds(plan)
    assert check_query_vars(kinds, list(range(D))) is False
    with pytest.raises(ValueError, match="input layer"):
        check_query_vars(kinds, [0, D])
    with pytest.raises(ValueError, match="at least one"):
        check_query_vars(kinds, [])
    mixed = variable_kinds(_case("plan_clt_mixed6_cp")[0])  # Categorical over the even variables, Gaussian over the odd ones
    with pytest.raises(NotImplementedError, match="mixes discrete and Gaussian"):
        check_query_vars(mixed, [0, 1])
    assert check_query_vars(mixed, [0, 2]) is False and check_query_vars(mixed, [1, 3]) is True


def test_leave_one_out_entry_points_are_exported_at_abi_51():
    from cirkit_amd import _capi as capi

    lib = capi.load()
    assert lib.ck_abi_version() == 51
    for n in NEW_ENTRY_POINTS:
        assert hasattr(lib, n) and n in capi.SIGNATURES
    assert lib.ck_loo_down_sum(0, 0, None, None, 1, 1, 1, 1, 1, None, None, None, 0, 1, None, None) == -1
    assert b"ck_loo_down_sum" in lib.ck_last_error()
