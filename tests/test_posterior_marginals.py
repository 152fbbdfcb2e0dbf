"""Posterior marginals (`HipCircuit.posterior_marginals`, cirkit_amd/posterior.py, cirkit_amd/csrc/ck_flow.hip; DESIGN.md
section 11).

The reference has no such query.  On the CPU the fp64 restatement of the flow contract (tests/posterior_restatement.py) is
pinned against brute force -- the quotient of two oracle marginal forwards per (variable, state) -- and, for Gaussian
leaves, against the oracle's autograd flows.  On the GPU the output is compared with that restatement, every row and every
entry.

GPU tolerance.  The yardstick is the restatement run in float32 (numpy, the same formulas) against its fp64 run ON THE
TEST'S OWN plan and evidence, computed by the test before it asserts (`_bound`): the GPU must be within 4 x that maximum
absolute error on probabilities (relative to 1 + |moment| for Gaussian means and variances), with a floor of 1e-6; the same
rule bounds |sum_c p - 1|, read as 4 x the larger of two fp32 figures, the entry error and the fp32 row sums' own distance from
1 (the looser reading: a sum of 256 entries cannot meet the per-entry bound, the fp32 restatement itself is at 1.5e-4 on the
784-pixel plan).  The factor 4 covers the different summation order of the MFMA tiles and the device's exp / log; nothing in the bound comes from what the GPU returns.  An fp32 evaluation carries the unit values v (down to about
-700 at an observed 256-state pixel) with an absolute error of ~|v| 2^-24 ~ 4e-5, which the flows exponentiate: the
yardstick is therefore ~1e-5 .. 1e-4 on the image plans and ~1e-6 on the 5-variable ones.  The Binomial plan gets its own
yardstick the same way: the restatement evaluates its log-pmf table by the reference's expression (torch's
Binomial.log_prob: c l - lgamma(c + 1) - lgamma(T - c + 1) - normaliser, terms of several hundred) with every term and step
in fp32, as the device's table does.  Measured yardsticks and GPU errors: DESIGN.md
section 11, "Posterior marginals".
"""
import os

import numpy as np
import pytest
import torch

from conftest import load_case
from posterior_restatement import posterior_restated
from test_mpe import PLANS, _case, _hc

DISCRETE_CPU = ["kat_bernoulli_f0o0", "kat_bernoulli_f0o1", "kat_bernoulli_f1o0", "kat_bernoulli_f1o1", "cfg1_rbt8",
                "binomial_qg6x6_k4", "plan_quadgraph_1x4x4_cp", "quadgraph_6x6_tucker_k4", "quadtree_4x4_kron_k3"]
NEW_ENTRY_POINTS = ("ck_flow_down_sum", "ck_flow_segment_add", "ck_flow_down_product", "ck_flow_leaf_categorical",
                    "ck_flow_leaf_gaussian")


def _states(plan) -> np.ndarray:
    """(D,) state count of every variable (0 for a Gaussian one)."""
    c = np.zeros(plan.num_variables, dtype=np.int64)
    for l in plan.layers:
        if l.type == "categorical":
            c[l.scope_idx[:, 0]] = int(l.config["num_categories"])
        elif l.type == "binomial":
            c[l.scope_idx[:, 0]] = int(l.config["total_count"]) + 1
    return c


def _random_evidence(plan, B, rng) -> np.ndarray:
    c = _states(plan)
    x = rng.normal(size=(B, plan.num_variables))
    d = c > 0
    x[:, d] = rng.integers(0, c[d], size=(B, int(d.sum())))
    return x


def _exact(plan, tensors):
    """The case with every Categorical `probs` given as a raw tensor normalised in fp64.  The oracle integrates such a layer
    to exactly log 1 whatever its rows sum to, and a fixture stored in fp32 sums to 1 +- 6e-8: without this the quotient of
    two forwards is not a distribution to better than that (measured: 9.7e-9 on the kat_bernoulli plans), whereas the
    contract divides every table row by its own sum.  Both sides of the comparison get the same tensors."""
    tensors = {k: np.asarray(v, dtype=np.float64) if np.asarray(v).dtype.kind == "f" else v for k, v in tensors.items()}
    for l in plan.layers:
        if l.type == "categorical" and "probs" in l.params and len(l.params["probs"].nodes) == 1:
            n = l.params["probs"].nodes[0]
            if n.op == "tensor":
                t = tensors[n.config["tensor"]]
                tensors[n.config["tensor"]] = t / t.sum(axis=-1, keepdims=True)
    return plan, tensors


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", DISCRETE_CPU)
def test_restatement_is_the_quotient_of_two_marginal_forwards(name):
    from oracle.torch_oracle import as_torch, evaluate_plan

    plan, tensors = _exact(*_case(name))
    D, B = plan.num_variables, 64
    rng = np.random.default_rng(11)
    x = _random_evidence(plan, B, rng)
    query = sorted(rng.choice(D, size=max(1, D // 2), replace=False).tolist())
    res = posterior_restated(plan, tensors, x, query)
    p = res["p"]
    assert np.isfinite(p).all()
    # Both sides in fp64: the oracle's Binomial takes torch.lgamma of an INTEGER tensor, which comes out in torch's default
    # dtype -- fp32 unless told otherwise, whatever the dtype of the parameters -- so the oracle runs with fp64 as the default.
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        _compare_with_brute_force(plan, tensors, x, query, res)
    finally:
        torch.set_default_dtype(default)


def _compare_with_brute_force(plan, tensors, x, query, res):
    from oracle.torch_oracle import as_torch, evaluate_plan

    D, B, p = plan.num_variables, x.shape[0], res["p"]
    tt = {k: v.double() for k, v in as_torch(tensors).items()}
    xt = torch.from_numpy(x.astype(np.int64))
    qmask = torch.zeros(D, dtype=torch.bool)
    qmask[query] = True
    log_ev = evaluate_plan(plan, tt, xt, integrate_mask=qmask)[:, 0, 0].numpy()
    assert np.abs(log_ev - res["logev"]).max() <= 1e-9 * (1 + np.abs(log_ev).max())
    states = _states(plan)
    for q, v in enumerate(query):
        C = int(states[v])
        xs = xt.repeat(C, 1)
        xs[:, v] = torch.arange(C).repeat_interleave(B)
        m = qmask.clone()
        m[v] = False
        joint = evaluate_plan(plan, tt, xs, integrate_mask=m)[:, 0, 0].numpy().reshape(C, B).T
        brute = np.exp(joint - log_ev[:, None])
        assert np.abs(p[:, q, :C] - brute).max() <= 1e-9, (v, np.abs(p[:, q, :C] - brute).max())
        assert (p[:, q, C:] == 0).all()


@pytest.mark.parametrize("name", ["kat_gaussian_f1o1", "pd_gauss_6x6_k4"])
def test_restated_gaussian_moments_equal_the_autograd_flows(name):
    from oracle.torch_oracle import as_torch, eval_param, evaluate_plan

    plan, tensors = _case(name)
    D, B = plan.num_variables, 64
    rng = np.random.default_rng(12)
    x = _random_evidence(plan, B, rng)
    query = sorted(rng.choice(D, size=max(1, D // 2), replace=False).tolist())
    res = posterior_restated(plan, tensors, x, query)
    tt = {k: v.double().requires_grad_(True) for k, v in as_torch(tensors).items()}
    qmask = torch.zeros(D, dtype=torch.bool)
    qmask[query] = True
    y, outs = evaluate_plan(plan, tt, torch.from_numpy(x), return_all=True, grad=True, integrate_mask=qmask)
    inputs = [j for j, l in enumerate(plan.layers) if l.inputs is None]
    grads = torch.autograd.grad(y[:, 0, 0].sum(), [outs[j] for j in inputs], allow_unused=True)
    s1 = np.zeros((B, len(query)))
    s2 = np.zeros((B, len(query)))
    for j, g in zip(inputs, grads):
        l = plan.layers[j]
        mean = eval_param(l.params["mean"], tt).detach().numpy()
        sd = eval_param(l.params["stddev"], tt).detach().numpy()
        for f in range(l.num_folds):
            v = int(l.scope_idx[f, 0])
            if v in query and g is not None:
                fl = g[f].numpy()  # (B, K): d log c / d log u, the flow
                assert np.abs(fl - res["flows"][j][f]).max() <= 1e-9
                s1[:, query.index(v)] += fl @ mean[f]
                s2[:, query.index(v)] += fl @ (sd[f] ** 2 + mean[f] ** 2)
    want = np.stack([s1, s2 - s1 * s1], axis=2)
    assert np.abs(res["p"] - want).max() <= 1e-9 * (1 + np.abs(want).max())
    assert np.abs(res["leaf_flow"] - 1).max() <= 1e-9


@pytest.mark.parametrize("name", DISCRETE_CPU + ["kat_gaussian_f1o1", "pd_gauss_6x6_k4"])
def test_restated_flows_are_conserved(name):
    plan, tensors = _case(name)
    D, B = plan.num_variables, 64
    rng = np.random.default_rng(13)
    x = _random_evidence(plan, B, rng)
    query = sorted(rng.choice(D, size=max(1, D // 2), replace=False).tolist())
    res = posterior_restated(plan, tensors, x, query)
    assert np.abs(res["leaf_flow"] - 1).max() <= 1e-9
    if _states(plan)[query].all():
        assert np.abs(res["p"].sum(2) - 1).max() <= 1e-9
    for fl in res["flows"]:
        assert fl.min() >= 0 and fl.max() <= 1 + 1e-9


def test_posterior_entry_points_are_exported_at_abi_51():
    from cirkit_amd import _capi as capi

    lib = capi.load()
    assert lib.ck_abi_version() == 51
    for n in NEW_ENTRY_POINTS:
        assert hasattr(lib, n) and n in capi.SIGNATURES


def test_shared_folds_have_several_consumers():
    from cirkit_amd.posterior import num_consumers

    for name in ("plan_quadgraph_1x4x4_cp", "quadgraph_6x6_tucker_k4", "pd_gauss_6x6_k4"):
        assert num_consumers(_case(name)[0]).max() > 1, name


# ------------------------------------------------------------------------------------------------------------ GPU
def _gauss(plan) -> bool:
    return any(l.type == "gaussian" for l in plan.layers)


def _err(got: np.ndarray, want: np.ndarray, gauss: bool) -> float:
    d = np.abs(got.astype(np.float64) - want)
    return float((d / (1 + np.abs(want))).max() if gauss else d.max())


def _bound(plan, tensors, x_np, query, want) -> tuple[float, float]:
    """4 x the errors of the fp32 restatement against the fp64 one on this plan and evidence, at least 1e-6: of its
    probabilities (moments), and of its row sums |sum_c p - 1|."""
    y32 = posterior_restated(plan, tensors, x_np, query, dtype=np.float32)["p"]
    yard = _err(y32, want, _gauss(plan))
    ysum = 0.0 if _gauss(plan) else float(np.abs(y32.astype(np.float64).sum(2) - 1).max())
    print(f"  fp32-restatement yardstick {yard:.3e}, of |sum_c p - 1| {ysum:.3e}")
    return max(4 * yard, 1e-6), max(4 * yard, 4 * ysum, 1e-6)


def _check(plan, tensors, x, query, p, log_ev=None, rows=None):
    x_np = x.cpu().numpy().astype(np.float64)
    p = p.cpu().numpy()
    if rows is not None:
        x_np, p = x_np[:rows], p[:rows]
    res = posterior_restated(plan, tensors, x_np, query)
    want = res["p"]
    assert p.shape == want.shape, (p.shape, want.shape)
    assert np.isfinite(p).all()  # (every row of sampled evidence has mass: nothing is left out of the comparison below)
    bound, bound_sum = _bound(plan, tensors, x_np, query, want)
    e = _err(p, want, _gauss(plan))
    print(f"  GPU error {e:.3e} (bound {bound:.3e})")
    assert e <= bound, (e, bound)
    if not _gauss(plan):
        s = float(np.abs(p.astype(np.float64).sum(2) - 1).max())
        print(f"  |sum_c p - 1| {s:.3e}")
        assert s <= bound_sum, (s, bound_sum)
    if log_ev is not None:
        lv = log_ev.cpu().numpy().astype(np.float64)[: want.shape[0]]
        assert np.abs(lv - res["logev"]).max() <= 1e-4 * (1 + np.abs(res["logev"]).max())
    return bound


def _query(kind, D):
    if kind == "random":
        return np.random.default_rng(5).random(D) < 0.5
    if kind == "lower_half":
        return np.arange(D) >= D // 2
    return np.ones(D, dtype=bool)


@pytest.mark.gpu
@pytest.mark.parametrize("mask_kind", ["random", "lower_half", "all"])
@pytest.mark.parametrize("name", PLANS)
def test_gpu_posterior_equals_restatement(hip_device, name, mask_kind):
    plan, tensors = _case(name)
    D = plan.num_variables
    N = 256 if name == "cfg2_qt784" else 1024
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(N, seed=77)  # evidence with mass
    mask = _query(mask_kind, D)
    if not mask.any():
        mask[0] = True
    query = np.nonzero(mask)[0].tolist()
    p, lv = hc.posterior_marginals(x, torch.from_numpy(mask), return_log_evidence=True)
    torch.cuda.synchronize()
    C = 2 if _gauss(plan) else int(_states(plan)[query].max())
    assert tuple(p.shape) == (N, len(query), C) and p.dtype == torch.float32 and p.device.type == "cuda"
    assert lv.shape == (N,) and lv.dtype == torch.float32
    _check(plan, tensors, x, query, p, lv)
    p2 = hc.posterior_marginals(x, query)  # ids instead of a mask; the query variables' own entries are ignored
    assert torch.equal(p2, p)
    xs = x.clone()
    xs[:, query[0]] = 0
    assert torch.equal(hc.posterior_marginals(xs, query), p)


@pytest.mark.gpu
def test_gpu_posterior_is_the_quotient_of_two_forwards(hip_device):
    plan, tensors = _case("cfg1_rbt8")
    D, N = plan.num_variables, 512
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(N, seed=3)
    query = [1, 2, 5, 6]
    p = hc.posterior_marginals(x, query)
    bound = _check(plan, tensors, x, query, p)
    base = hc(x, integrate_vars=query)[:, 0, 0].clone()
    for q, v in enumerate(query):
        rest = [u for u in query if u != v]
        for c in range(int(_states(plan)[v])):
            xc = x.clone()
            xc[:, v] = c
            lq = (hc(xc, integrate_vars=rest)[:, 0, 0] - base).double().cpu().numpy()
            got = p[:, q, c].double().cpu().numpy()
            big = got > 1e-3  # (log space where p is not tiny)
            # (the same bound, taken in log space, plus the fp32 rounding of the two forwards' values: 2^-18 (1 + |log q|))
            assert np.abs(np.log(got[big]) - lq[big]).max() <= bound + 4e-6 * (1 + np.abs(lq[big]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2_qt784", "pd_gauss_6x6_k4"])
def test_gpu_posterior_chunking_does_not_change_results(hip_device, name):
    plan, tensors = _case(name)
    D, B = plan.num_variables, 300
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(B, seed=8)
    query = np.nonzero(np.random.default_rng(4).random(D) < 0.25)[0].tolist()
    res = [hc.posterior_marginals(x, query, return_log_evidence=True, rows_per_chunk=r) for r in (None, 1, 7)]
    for p, lv in res[1:]:
        assert torch.equal(p, res[0][0]) and torch.equal(lv, res[0][1])
    p, lv = hc.posterior_marginals(x, query, return_log_evidence=True)
    assert torch.equal(p, res[0][0]) and torch.equal(lv, res[0][1])


@pytest.mark.gpu
def test_gpu_posterior_shared_folds(hip_device):
    from cirkit_amd.posterior import num_consumers

    for name in ("plan_quadgraph_1x4x4_cp", "pd_gauss_6x6_k4"):
        plan, tensors = _case(name)
        hc = _hc(plan, tensors, hip_device)
        assert num_consumers(hc.plan).max() > 1  # (the plan the device walks, not only the user's)
        x = hc.sample(128, seed=2)
        query = list(range(0, plan.num_variables, 3))
        _check(plan, tensors, x, query, hc.posterior_marginals(x, query))


@pytest.mark.gpu
def test_gpu_posterior_impossible_evidence_and_point_mass(hip_device):
    plan, tensors = _case("cfg1_rbt8")
    D, N = plan.num_variables, 512
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
    query = [u for u in range(D) if u != var][::2]
    p, lv = hc.posterior_marginals(x, query, return_log_evidence=True)
    assert bool((lv[bad] == -np.inf).all()) and bool(torch.isfinite(lv[~bad]).all())
    assert bool(torch.isnan(p[bad]).all())
    _check(plan, tensors, x[~bad], query, p[~bad], lv[~bad])
    # the point mass queried instead of observed: exactly the point mass, no NaN from 0 * inf
    p = hc.posterior_marginals(x, [var])
    want = torch.zeros(int(_states(plan)[var]), device=hip_device)
    want[cc] = 1.0
    assert bool(torch.isfinite(p).all())
    assert bool((p[:, 0, :][:, want == 0] == 0).all())  # exactly 0 off the point
    _check(plan, tensors, x, [var], p)  # (on it: the flow that reaches the variable, 1 within the row-sum bound)


@pytest.mark.gpu
def test_gpu_posterior_out_of_range_evidence_is_reported_and_does_not_stick(hip_device):
    plan, tensors = _case("cfg2_qt784")  # Categorical-256
    D, N = plan.num_variables, 128
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(N, seed=4)
    query = list(range(D // 2, D, 8))
    bad = x.clone()
    bad[5, 10] = 300  # an observed category out of range
    keep = torch.arange(N, device=hip_device) != 5
    res = [hc.posterior_marginals(bad, query, return_log_evidence=True, rows_per_chunk=r) for r in (None, 1, 7)]
    for p, lv in res:  # that row alone is NaN, whatever the chunking; every other row is the restatement's
        assert bool(torch.isnan(p[5]).all()) and bool(torch.isnan(lv[5]))
        assert bool(torch.isfinite(p[keep]).all()) and bool(torch.isfinite(lv[keep]).all())
        assert torch.equal(p[keep], res[0][0][keep]) and torch.equal(lv[keep], res[0][1][keep])
    _check(plan, tensors, bad[keep], query, res[0][0][keep], res[0][1][keep])
    with pytest.raises(IndexError):  # reported where hc(x) reports it, and cleared by the check
        hc.check_inputs()
    hc.check_inputs()
    p = hc.posterior_marginals(x, query)
    _check(plan, tensors, x, query, p)
    hc.check_inputs()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_gpu_posterior_follows_training_steps(hip_device, fused):
    from cirkit_amd.training import HipTrainer

    plan, tensors, g = load_case("cfg2_qt784")
    xb = torch.from_numpy(g["x"].astype(np.int64)).to(hip_device)
    tr = HipTrainer(plan, tensors, device=hip_device, lr=0.05, fused=None if fused else False)
    assert tr.fused == fused
    query = list(range(392, 784, 16))
    before = tr.circuit.posterior_marginals(xb, query).clone()
    for _ in range(3):
        tr.step(xb)
    after, la = tr.circuit.posterior_marginals(xb, query, return_log_evidence=True)
    assert not torch.equal(before, after)
    fresh, lf = _hc(plan, tr.parameters(), hip_device).posterior_marginals(xb, query, return_log_evidence=True)
    assert torch.equal(after, fresh) and torch.equal(la, lf)


@pytest.mark.gpu
def test_gpu_posterior_config4_default_chunks(hip_device):
    plan, tensors = _case("cfg4_pd784")
    D, B = plan.num_variables, 2048
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(B, seed=12)
    query = np.nonzero(np.arange(D) >= D // 2)[0].tolist()
    p, lv = hc.posterior_marginals(x, query, return_log_evidence=True)
    assert tuple(p.shape) == (B, len(query), 2)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(lv).all())
    _check(plan, tensors, x, query, p, lv, rows=32)


@pytest.mark.gpu
def test_gpu_posterior_refusals(hip_device):
    plan, tensors = _case("cfg5_sos_c_k32")
    hc = _hc(plan, tensors, hip_device)
    with pytest.raises(ValueError, match="lse-sum"):
        hc.posterior_marginals(torch.zeros((4, plan.num_variables), dtype=torch.int64, device=hip_device), [0])
    plan, tensors = _case("cfg1_rbt8")
    D = plan.num_variables
    hc = _hc(plan, tensors, hip_device)
    x = torch.zeros((4, D), dtype=torch.int64, device=hip_device)
    with pytest.raises(ValueError):
        hc.posterior_marginals(x, torch.ones((4, D), dtype=torch.bool))  # a (B, D) mask: the output would be ragged
    with pytest.raises(ValueError):
        hc.posterior_marginals(x, torch.ones((D + 1,), dtype=torch.bool))
    with pytest.raises(ValueError):
        hc.posterior_marginals(x, [D])
    assert hc._sampler._key is None and hc._sampler._zc is None
    # a query variable no input layer covers, and a query set mixing discrete and Gaussian variables
    import copy

    wide = copy.deepcopy(plan)
    wide.num_variables = D + 1
    hw = _hc(wide, tensors, hip_device)
    xw = torch.zeros((4, D + 1), dtype=torch.int64, device=hip_device)
    with pytest.raises(ValueError, match="input layer"):
        hw.posterior_marginals(xw, [0, D])
    assert hw._sampler._key is None and hw._sampler._zc is None
    mixed, mt = _case("plan_clt_mixed6_cp")  # Categorical over the even variables, Gaussian over the odd ones
    hm = _hc(mixed, mt, hip_device)
    xm = torch.zeros((4, mixed.num_variables), dtype=torch.float32, device=hip_device)
    with pytest.raises(NotImplementedError):
        hm.posterior_marginals(xm, [0, 1])
    assert hm._sampler._key is None and hm._sampler._zc is None
    assert tuple(hm.posterior_marginals(xm, [0, 2]).shape) == (4, 2, 3)  # (each kind on its own is served)
    assert tuple(hm.posterior_marginals(xm, [1]).shape) == (4, 1, 2)
