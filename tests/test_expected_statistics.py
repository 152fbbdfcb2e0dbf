"""Expected statistics (`HipCircuit.expected_statistics`, cirkit_amd/expected.py, cirkit_amd/csrc/ck_stats.hip; DESIGN.md
section 11, "Expected statistics").

The reference has no such query.  On the CPU the fp64 restatement of the contract (tests/statistics_restatement.py) is pinned
against the oracle's autograd (the expected edge flow of a weight is w dL/dw, the flow of a unit dL/d(its output)), against
its own conservation identities, and against the one property that makes it an E-step: one EM step does not lower the
likelihood.  On the GPU the output is compared with that restatement, every entry of every layer.

GPU tolerance: `_bound`'s rule of tests/test_posterior_marginals.py.  The error of a field is max |got - want| / (1 + |want|);
the yardstick is that error of the restatement run in float32 against its fp64 run ON THE TEST'S OWN plan and evidence,
computed before anything is asserted; the GPU must be within 4 x the yardstick, with a floor of 1e-6.  Nothing in the bound
comes from what the GPU returns.  Measured yardsticks and GPU errors: DESIGN.md section 11, "Expected statistics".
"""
import functools
from unittest import mock

import numpy as np
import pytest
import torch

from statistics_restatement import normalised_restated, statistics_restated
from test_mpe import PLANS, _case, _hc
from test_posterior_marginals import _states

SMALL = {"qt2_cp_k32": ("quad-tree-2", "cp", 32), "qt2_cpt_k64": ("quad-tree-2", "cp-t", 64),
         "qg_cp_k32": ("quad-graph", "cp", 32), "qt2_tucker_k32": ("quad-tree-2", "tucker", 32)}
GPU_PLANS = list(SMALL) + [p for p in PLANS if p != "cfg2_qt784"]
CPU_PLANS = ["kat_bernoulli_f0o1", "kat_bernoulli_f1o1", "kat_gaussian_f1o1", "cfg1_rbt8", "binomial_qg6x6_k4",
             "quadtree_4x4_kron_k3", "plan_quadgraph_1x4x4_cp", "quadgraph_6x6_tucker_k4", "pd_gauss_6x6_k4"]
NEW_ENTRY_POINTS = ("ck_stats_edge_sum", "ck_stats_leaf_categorical", "ck_stats_leaf_gaussian", "ck_stats_unit_sum")
FIELDS = ("edge", "leaf", "unit")


@functools.lru_cache(maxsize=None)
def _small(name):
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import image_data

    rg, sp, k = SMALL[name]
    plan = image_data((1, 4, 4), rg, num_input_units=k, sum_product_layer=sp, num_sum_units=k)
    return plan, init_plan_tensors(plan, seed=5)


def _any_case(name):
    return _small(name) if name in SMALL else _case(name)


def _random_x(plan, B, rng):
    c = _states(plan)
    x = rng.normal(size=(B, plan.num_variables))
    d = c > 0
    x[:, d] = rng.integers(0, c[d], size=(B, int(d.sum())))
    return x


def _root_layer(plan):
    from cirkit_amd.plan import resolve_fold_index

    return int(resolve_fold_index(plan.output, [l.num_folds for l in plan.layers]).reshape(-1, 2)[0][0])


def _var_unit_sums(plan, unit) -> np.ndarray:
    """(D,) the sum of `unit` over the input folds of each variable."""
    s = np.zeros(plan.num_variables)
    for j, l in enumerate(plan.layers):
        if l.inputs is None:
            np.add.at(s, l.scope_idx[:, 0], np.asarray(unit[j], dtype=np.float64).sum(axis=1))
    return s


def _violations(plan, res, vals=None) -> dict:
    """The four conservation identities, each as the largest |difference|."""
    unit = [np.asarray(u, dtype=np.float64) for u in res["unit"]]
    out = {"edge": 0.0, "leaf": 0.0}
    for j, e in res["edge"].items():
        d = np.abs(np.asarray(e, dtype=np.float64).sum(-1) - unit[j])
        if vals is not None:  # (a unit whose value is not finite in some row keeps its flow but gives no edge flow there)
            d = d[np.isfinite(vals[j]).all(axis=1)]
        out["edge"] = max(out["edge"], float(d.max()) if d.size else 0.0)
    for j, e in res["leaf"].items():
        tot = np.asarray(e, dtype=np.float64)
        tot = tot[..., 0] if plan.layers[j].type == "gaussian" else tot.sum(-1)
        out["leaf"] = max(out["leaf"], float(np.abs(tot - unit[j]).max()))
    out["root"] = float(abs(unit[_root_layer(plan)].sum() - res["rows"]))
    out["vars"] = float(np.abs(_var_unit_sums(plan, unit) - res["rows"]).max())
    return out


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", CPU_PLANS)
def test_restatement_equals_the_autograd_of_the_oracle(name):
    import oracle.torch_oracle as to

    plan, tensors = _case(name)
    D, B = plan.num_variables, 64
    rng = np.random.default_rng(21)
    x = _random_x(plan, B, rng)
    missing = sorted(rng.choice(D, size=D // 2, replace=False).tolist())
    res = statistics_restated(plan, tensors, x, missing)
    assert res["rows"] == B
    tt = {k: v.double().requires_grad_(True) for k, v in to.as_torch(tensors).items()}
    seen = []
    real = to.eval_param

    def recording(pg, tensors_):
        t = real(pg, tensors_)
        if t.requires_grad:
            t.retain_grad()
        seen.append((id(pg), t))
        return t

    mask = torch.zeros(D, dtype=torch.bool)
    mask[missing] = True
    gauss = any(l.type == "gaussian" for l in plan.layers)
    xt = torch.from_numpy(x if gauss else x.astype(np.int64))
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # (the oracle's Binomial: tests/test_posterior_marginals.py explains)
    try:
        with mock.patch.object(to, "eval_param", recording):
            y, outs = to.evaluate_plan(plan, tt, xt, return_all=True, grad=True, integrate_mask=mask)
        for o in outs:
            o.retain_grad()
        y[:, 0, 0].sum().backward()
    finally:
        torch.set_default_dtype(default)
    by_graph = dict(seen)
    near = lambda got, want: np.abs(got - want).max() <= 1e-9 * (1 + np.abs(want).max())  # noqa: E731
    for j, l in enumerate(plan.layers):
        g = outs[j].grad
        flow = np.zeros((l.num_folds, B, l.num_output_units)) if g is None else g.numpy()
        assert near(res["unit"][j], flow.sum(axis=1)), (j, l.type)
        if j in res["edge"]:
            w = by_graph[id(l.params["weight"])]
            wg = np.zeros(w.shape) if w.grad is None else w.grad.numpy()
            assert near(res["edge"][j], (w.detach().numpy() * wg).reshape(res["edge"][j].shape)), (j, l.type)
        elif l.inputs is None and l.type != "gaussian":  # the observed part: the flows histogrammed by the row's category
            for f in range(l.num_folds):
                v = int(l.scope_idx[f, 0])
                if v in missing:
                    continue
                C = res["leaf"][j].shape[2]
                hist = np.stack([flow[f][x[:, v].astype(np.int64) == c].sum(axis=0) for c in range(C)], axis=1)
                assert near(res["leaf"][j][f], hist), (j, f)


@pytest.mark.parametrize("name", CPU_PLANS)
def test_restated_statistics_are_conserved(name):
    plan, tensors = _case(name)
    D, B = plan.num_variables, 64
    rng = np.random.default_rng(22)
    x = _random_x(plan, B, rng)
    x[rng.random((B, D)) < 0.3] = np.nan if _states(plan).min() == 0 else -1  # per-row sentinels
    res = statistics_restated(plan, tensors, x, [0])
    for what, v in _violations(plan, res, res["vals"]).items():
        assert v <= 1e-9 * (1 + B), (what, v)


def _em_case(D=6, C=3, K=3):
    """A plan whose sum weights and Categorical logits are raw tensors, normalised: log c(x) is a log-likelihood."""
    from cirkit_amd.templates import InputSpec, build_plan, random_binary_tree

    plan = build_plan(random_binary_tree(D), input_layer=InputSpec("categorical", C), num_input_units=K, num_sum_units=K,
                      sum_activation="none", input_activation="none")
    rng = np.random.default_rng(7)
    tensors = {}
    for l in plan.layers:
        for g in l.params.values():
            assert len(g.nodes) == 1 and g.nodes[0].op == "tensor"
            n = g.nodes[0].config["tensor"]
            t = rng.random(plan.tensors[n][0]) + 0.1
            t = t / t.sum(axis=-1, keepdims=True)
            tensors[n] = np.log(t) if l.inputs is None else t
    return plan, tensors


@pytest.mark.parametrize("missing_fraction", [0.0, 1.0 / 3.0])
def test_one_em_step_does_not_lower_the_likelihood(missing_fraction):
    from oracle.torch_oracle import as_torch, evaluate_plan

    plan, tensors = _em_case()
    D, B = plan.num_variables, 64
    rng = np.random.default_rng(23)
    x = rng.integers(0, 3, size=(B, D)).astype(np.float64)
    miss = rng.random((B, D)) < missing_fraction
    miss[miss.all(axis=1), 0] = False
    xs = np.where(miss, -1.0, x)

    def mean_ll(t):
        tt = {k: v.double() for k, v in as_torch(t).items()}
        y = evaluate_plan(plan, tt, torch.from_numpy(x.astype(np.int64)), integrate_mask=torch.from_numpy(miss))
        return float(y[:, 0, 0].mean())

    before = mean_ll(tensors)
    res = statistics_restated(plan, tensors, xs)
    target = normalised_restated(plan, res)
    new = dict(tensors)
    for j, l in enumerate(plan.layers):
        (g,) = l.params.values()
        with np.errstate(divide="ignore"):
            new[g.nodes[0].config["tensor"]] = np.log(target[j]) if l.inputs is None else target[j]
    after = mean_ll(new)
    assert np.isfinite(before) and np.isfinite(after)
    assert after >= before - 1e-9, (before, after)
    assert after > before  # (random parameters are no fixed point)


def test_statistics_entry_points_are_exported_at_abi_51():
    from cirkit_amd import _capi as capi

    lib = capi.load()
    assert lib.ck_abi_version() == 51
    for n in NEW_ENTRY_POINTS:
        assert hasattr(lib, n) and n in capi.SIGNATURES


def test_statistics_invalid_arguments_return_status_and_message():
    from cirkit_amd import _capi as capi

    lib = capi.load()
    p = 64  # (never dereferenced: validation comes before any launch)
    calls = {
        "ck_stats_edge_sum": [
            (capi.CK_SAMPLE_SUM, 0, None, p, 1, 1, 4, 4, 4, p, p, p, 0, p, 8, p, None, 0, None),  # null child
            (capi.CK_SAMPLE_SUM, 0, p, p, 1, 1, 4, 4, 4, p, p, p, 0, p, 0, p, None, 0, None),  # no rows
            (capi.CK_SAMPLE_HADAMARD, 0, p, p, 1, 1, 4, 4, 4, p, p, p, 0, p, 8, p, None, 0, None),  # not a sum-type layer
            (capi.CK_SAMPLE_CPT, 0, p, p, 1, 2, 4, 4, 8, p, p, p, 0, p, 8, p, None, 0, None),  # entries do not match
            (capi.CK_SAMPLE_SUM, 0, p, p, 1, 1, 4, 4, 4, p, p, p, 0, p, 4096, p, None, 0, None),  # row slices, no scratch
        ],
        "ck_stats_leaf_categorical": [
            (p, None, 1, 4, 3, p, 0, 5, p, p, 0, p, 8, p, None),
            (p, p, 1, 0, 3, p, 0, 5, p, p, 0, p, 8, p, None),
        ],
        "ck_stats_leaf_gaussian": [
            (p, p, p, 1, 4, None, 5, p, p, 0, p, 8, p, None),
            (p, p, p, 1, 4, p, 5, p, p, -1, p, 8, p, None),
        ],
        "ck_stats_unit_sum": [
            (p, p, p, p, 3, None, 8, p, None),
            (p, p, p, p, 0, p, 8, p, None),
        ],
    }
    for name, cases in calls.items():
        fn = getattr(lib, name)
        for args in cases:
            assert fn(*args) == -1, (name, args)
            assert name in lib.ck_last_error().decode()
            with pytest.raises(ValueError, match=name):
                capi.call(name, *args)


# ------------------------------------------------------------------------------------------------------------ GPU
def _np(st) -> dict:
    return {"edge": {j: t.cpu().numpy() for j, t in st.edge.items()}, "leaf": {j: t.cpu().numpy() for j, t in st.leaf.items()},
            "unit": [t.cpu().numpy() for t in st.unit], "logev": st.log_evidence.cpu().numpy(), "rows": int(st.rows)}


def _items(res, field):
    return list(res[field].items()) if isinstance(res[field], dict) else list(enumerate(res[field]))


def _errors(got, want) -> dict:
    out = {}
    for field in FIELDS:
        g, w = dict(_items(got, field)), dict(_items(want, field))
        assert sorted(g) == sorted(w), (field, sorted(g), sorted(w))
        e = 0.0
        for j in w:
            assert g[j].shape == w[j].shape, (field, j, g[j].shape, w[j].shape)
            e = max(e, float((np.abs(g[j].astype(np.float64) - w[j]) / (1 + np.abs(w[j]))).max()))
        out[field] = e
    return out


def _add(a, b) -> dict:
    return {"edge": {j: a["edge"][j].astype(np.float64) + b["edge"][j] for j in a["edge"]},
            "leaf": {j: a["leaf"][j].astype(np.float64) + b["leaf"][j] for j in a["leaf"]},
            "unit": [u.astype(np.float64) + v for u, v in zip(a["unit"], b["unit"])], "rows": a["rows"] + b["rows"]}


def _references(plan, tensors, x_np, missing):
    """The fp64 restatement, the per-field bounds (4 x the fp32 restatement's error, at least 1e-6) and the fp32
    restatement's own violations of the conservation identities."""
    want = statistics_restated(plan, tensors, x_np, missing)
    y32 = statistics_restated(plan, tensors, x_np, missing, dtype=np.float32)
    yard = _errors(y32, want)
    print("  fp32-restatement yardstick " + ", ".join(f"{k} {v:.3e}" for k, v in yard.items()))
    return want, {k: max(4 * v, 1e-6) for k, v in yard.items()}, _violations(plan, y32, want["vals"])


def _check(plan, tensors, x, missing, st, keep=None):
    x_np = x.cpu().numpy().astype(np.float64)
    if keep is not None:
        x_np = x_np[keep]
    want, bound, viol32 = _references(plan, tensors, x_np, missing)
    got = _np(st)
    for field in FIELDS:
        for _, t in _items(got, field):
            assert t.dtype == np.float32 and np.isfinite(t).all()
    err = _errors(got, want)
    print("  GPU error " + ", ".join(f"{k} {v:.3e} (bound {bound[k]:.3e})" for k, v in err.items()))
    for field in FIELDS:
        assert err[field] <= bound[field], (field, err[field], bound[field])
    assert got["rows"] == want["rows"]
    return want, bound, viol32, got


def _pattern(kind, plan, x, rng):
    """(evidence, missing variables) of a missing pattern: none, a random half of the variables, per-row sentinels."""
    D = plan.num_variables
    if kind == "half":
        return x, sorted(rng.choice(D, size=D // 2, replace=False).tolist())
    if kind == "sentinels":
        x = x.clone()
        m = torch.from_numpy(rng.random(tuple(x.shape)) < 1.0 / 3.0).to(x.device)
        x[m] = float("nan") if x.dtype.is_floating_point else -1
    return x, None


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["none", "half", "sentinels"])
@pytest.mark.parametrize("name", GPU_PLANS)
def test_gpu_statistics_equal_restatement(hip_device, name, pattern):
    plan, tensors = _any_case(name)
    hc = _hc(plan, tensors, hip_device)
    x, missing = _pattern(pattern, plan, hc.sample(70, seed=31), np.random.default_rng(32))
    st = hc.expected_statistics(x, missing)
    assert st.log_evidence.shape == (70,) and st.rows.dtype == torch.int64 and st.rows.dim() == 0
    want, bound, viol32, got = _check(plan, tensors, x, missing or (), st)
    assert np.abs(got["logev"] - want["logev"]).max() <= 1e-4 * (1 + np.abs(want["logev"]).max())
    # conservation on the device output: 4 x the fp32 restatement's own violation, at least 1e-6 (1 + rows)
    viol = _violations(plan, got, want["vals"])
    print("  conservation " + ", ".join(f"{k} {v:.3e} (fp32 restatement {viol32[k]:.3e})" for k, v in viol.items()))
    for what, v in viol.items():
        assert v <= max(4 * viol32[what], 1e-6 * (1 + want["rows"])), (what, v, viol32[what])


@pytest.mark.gpu
def test_gpu_statistics_config2(hip_device):
    plan, tensors = _case("cfg2_qt784")
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(64, seed=33)
    missing = list(range(plan.num_variables // 2, plan.num_variables))
    _check(plan, tensors, x, missing, hc.expected_statistics(x, missing))


@pytest.mark.gpu
def test_gpu_statistics_row_and_slice_edges(hip_device):
    plan, tensors = _small("qt2_cp_k32")
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(65, seed=34)
    missing = [3, 4, 9]
    parts = {}
    for B in (1, 2, 31, 33, 65):
        parts[B] = _check(plan, tensors, x[:B], missing, hc.expected_statistics(x[:B], missing))
    _, bound, _, whole = parts[65]
    tail = _np(hc.expected_statistics(x[33:], missing))
    err = _errors(whole, _add(parts[33][3], tail))
    for field in FIELDS:
        assert err[field] <= bound[field], (field, err[field], bound[field])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qt2_cp_k32", "qg_cp_k32", "pd_gauss_6x6_k4"])
def test_gpu_statistics_are_deterministic(hip_device, name):
    plan, tensors = _any_case(name)
    hc = _hc(plan, tensors, hip_device)
    x, _ = _pattern("sentinels", plan, hc.sample(70, seed=35), np.random.default_rng(36))
    a, b = hc.expected_statistics(x, [1]), hc.expected_statistics(x, [1])
    for field in FIELDS:  # (leaf too: the histogram is filled in row order, no atomics)
        for (_, s), (_, t) in zip(_items(vars(a), field), _items(vars(b), field)):
            assert torch.equal(s, t), field
    c = hc.expected_statistics(x, [1], rows_per_chunk=7)
    assert torch.equal(c.log_evidence, a.log_evidence) and torch.equal(c.rows, a.rows)
    _, bound, _ = _references(plan, tensors, x.cpu().numpy().astype(np.float64), [1])
    err = _errors(_np(c), {k: v for k, v in _np(a).items()})
    for field in FIELDS:
        assert err[field] <= bound[field], (field, err[field], bound[field])


@pytest.mark.gpu
def test_gpu_statistics_impossible_evidence_and_point_mass(hip_device):
    plan, tensors = _case("cfg1_rbt8")
    D, N = plan.num_variables, 64
    hc = _hc(plan, tensors, hip_device)
    cat = plan.layers[0]
    name = cat.params["probs"].nodes[0].config["tensor"]
    v = np.array(hc.store.export(name), dtype=np.float32)
    f, cc = 3, 1
    v[f] = -np.inf
    v[f, ..., cc] = 0.0  # a point mass in one Categorical fold
    hc.store.set(name, v)
    tensors = dict(tensors)
    tensors[name] = v
    var = int(cat.scope_idx[f, 0])
    x = hc.sample(N, seed=9)
    assert bool((x[:, var] == cc).all())
    bad = torch.arange(N, device=hip_device) % 2 == 1
    x[bad, var] = cc + 1  # contradicting evidence in half the rows
    st = hc.expected_statistics(x)
    assert int(st.rows) == N // 2
    assert bool((st.log_evidence[bad] == -np.inf).all()) and bool(torch.isfinite(st.log_evidence[~bad]).all())
    _check(plan, tensors, x, (), st, keep=(~bad).cpu().numpy())  # (finite everywhere, and the live half's statistics)
    _check(plan, tensors, x[~bad], [var], hc.expected_statistics(x[~bad], [var]))  # the point mass integrated out


@pytest.mark.gpu
def test_gpu_statistics_out_of_range_evidence_is_reported_and_does_not_stick(hip_device):
    plan, tensors = _case("cfg1_rbt8")
    N = 64
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(N, seed=4)
    bad = x.clone()
    bad[5, 2] = int(_states(plan)[2]) + 3  # an observed category out of range
    keep = np.arange(N) != 5
    st = hc.expected_statistics(bad)
    assert int(st.rows) == N - 1 and bool(torch.isnan(st.log_evidence[5]))
    _check(plan, tensors, bad, (), st, keep=keep)
    with pytest.raises(IndexError):
        hc.check_inputs()
    hc.check_inputs()
    _check(plan, tensors, x, (), hc.expected_statistics(x))
    hc.check_inputs()


@pytest.mark.gpu
def test_gpu_statistics_have_the_user_plans_shapes(hip_device):
    for name in ("quadtree_4x4_kron_k3", "cfg1_rbt8", "quadgraph_6x6_tucker_k4"):
        plan, tensors = _case(name)
        hc = _hc(plan, tensors, hip_device)
        st = hc.expected_statistics(hc.sample(16, seed=2))
        for j, l in enumerate(plan.layers):
            assert tuple(st.unit[j].shape) == (l.num_folds, l.num_output_units)
            if l.inputs is None:
                C = 3 if l.type == "gaussian" else int(_states(plan)[l.scope_idx[0, 0]])
                assert tuple(st.leaf[j].shape) == (l.num_folds, l.num_output_units, C)
            elif "weight" in l.params:
                M = {"sum": l.arity * l.num_input_units, "cpt": l.num_input_units, "tucker": l.num_input_units ** 2}[l.type]
                assert tuple(st.edge[j].shape) == (l.num_folds, l.num_output_units, M)
                w = st.normalised(0.5)[j]
                assert tuple(w.shape) == tuple(st.edge[j].shape)
                tot = w.sum(-1)
                assert bool(((tot - 1).abs() <= 1e-5).logical_or(tot == 0).all())
    assert any(a.num_output_units != b.num_output_units for a, b in zip(hc.plan.layers, hc.user_plan.layers))


@pytest.mark.gpu
def test_gpu_statistics_follow_parameter_changes(hip_device):
    plan, tensors = _small("qt2_cp_k32")
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(70, seed=37)
    before = hc.expected_statistics(x, [2])
    j = next(j for j, l in enumerate(plan.layers) if l.type == "sum")
    name = next(n.config["tensor"] for n in plan.layers[j].params["weight"].nodes if n.op == "tensor")
    new = dict(tensors)
    new[name] = np.random.default_rng(38).normal(size=np.asarray(tensors[name]).shape).astype(np.float32)
    hc.store.set(name, new[name])
    after = hc.expected_statistics(x, [2])
    fresh = _hc(plan, new, hip_device).expected_statistics(x, [2])
    assert not torch.equal(before.edge[j], after.edge[j])
    for field in FIELDS:
        for (_, s), (_, t) in zip(_items(vars(after), field), _items(vars(fresh), field)):
            assert torch.equal(s, t), field
    assert torch.equal(after.log_evidence, fresh.log_evidence)


@pytest.mark.gpu
def test_gpu_statistics_refusals(hip_device):
    plan, tensors = _case("cfg5_sos_c_k32")
    hc = _hc(plan, tensors, hip_device)
    with pytest.raises(ValueError, match="lse-sum"):
        hc.expected_statistics(torch.zeros((4, plan.num_variables), dtype=torch.int64, device=hip_device))
    plan, tensors = _case("cfg1_rbt8")
    D = plan.num_variables
    hc = _hc(plan, tensors, hip_device)
    x = torch.zeros((4, D), dtype=torch.int64, device=hip_device)
    for wrong in (torch.ones((4, D), dtype=torch.bool), torch.ones((D + 1,), dtype=torch.bool), [D]):
        with pytest.raises(ValueError):
            hc.expected_statistics(x, wrong)
    with pytest.raises(ValueError):
        hc.expected_statistics(x[0])
    with pytest.raises(ValueError):
        hc.expected_statistics(x, rows_per_chunk=0)
    assert hc._sampler._key is None and hc._sampler._zc is None
    from cirkit_amd.expected import ExpectedStatisticsQuery

    st = ExpectedStatisticsQuery(hc)(x, missing_vars=torch.arange(D) >= D // 2)
    assert int(st.rows) == 4
