"""The numpy restatement of the M-step (tests/em_restatement.py) pinned on the CPU, before the GPU is compared with it
(tests/test_em_training.py): at step_size = 1 the new raw tensors MEAN the closed-form targets of
`normalised_restated`, EM never lowers the fp64 likelihood, a half step is the midpoint, rows without statistics stay, the
clamps keep the raw values finite.  DESIGN.md section 11, "EM training"."""
import functools

import numpy as np
import pytest
import torch

from em_restatement import CLAMP, em_restated, normalised_parameters
from statistics_restatement import normalised_restated, statistics_restated
from test_expected_statistics import _em_case, _random_x
from test_mpe import _case

TEMPLATES = {"gauss_qt2_k4": ("quad-tree-2", "gaussian", 4), "binom_qt2_k4": ("quad-tree-2", "binomial", 4),
             "qg_cp_k3": ("quad-graph", "categorical", 3)}


@functools.lru_cache(maxsize=None)
def template(name):
    """The three extra template plans of the EM tests: a Gaussian and a Binomial 4 x 4 image plan, and a 3-unit plan (padded
    to 32 units on the device)."""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import image_data

    rg, il, k = TEMPLATES[name]
    plan = image_data((1, 4, 4), rg, input_layer=il, num_input_units=k, sum_product_layer="cp", num_sum_units=k)
    return plan, init_plan_tensors(plan, seed=6)


def _softmax_case(D=6, C=3, K=3):
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import InputSpec, build_plan, random_binary_tree

    plan = build_plan(random_binary_tree(D), input_layer=InputSpec("categorical", C), num_input_units=K, num_sum_units=K)
    return plan, init_plan_tensors(plan, seed=8)


def _any(name):
    if name == "em_bare":
        return _em_case()
    if name == "em_softmax":
        return _softmax_case()
    return template(name) if name in TEMPLATES else _case(name)


def mean_ll(plan, tensors, x, miss) -> float:
    """The fp64 mean log-likelihood of the rows of x with the entries `miss` marks integrated out (the oracle)."""
    from oracle.torch_oracle import as_torch, evaluate_plan

    tt = {k: v.double() for k, v in as_torch({k: np.asarray(v) for k, v in tensors.items()}).items()}
    gauss = any(l.type == "gaussian" for l in plan.layers)
    xt = torch.from_numpy(np.where(miss, 0, x) if gauss else np.where(miss, 0, x).astype(np.int64))
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # (the oracle's Binomial: tests/test_posterior_marginals.py explains)
    try:
        y = evaluate_plan(plan, tt, xt, integrate_mask=torch.from_numpy(miss))
    finally:
        torch.set_default_dtype(default)
    return float(y[:, 0, 0].mean())


def _direct_targets(plan, res) -> dict:
    """{(layer, parameter): target} of `ExpectedStatistics.normalised` restated: `normalised_restated` for the sum-type and
    Categorical layers, the moment formulas for the Gaussian and Binomial ones."""
    tg = normalised_restated(plan, res)
    out = {}
    for j, l in enumerate(plan.layers):
        if j in tg:
            (pn,) = l.params
            t = tg[j]
            if l.params[pn].ops[-1] == "mixing_weight":
                F, K, M = t.shape
                k = np.arange(K)
                t = np.stack([t[:, k, h * K + k] for h in range(M // K)], axis=-1)
            out[(j, pn)] = t
        elif l.type == "gaussian":
            s = res["leaf"][j]
            mean = s[..., 1] / s[..., 0]
            out[(j, "mean")] = mean
            c = l.params["stddev"].nodes[1].config  # (the scaled sigmoid reaches (vmin, vmax) only: the contract's clamp)
            lo, hi = c["vmin"], c["vmax"]
            sd = np.sqrt(np.maximum(s[..., 2] / s[..., 0] - mean * mean, 0))
            out[(j, "stddev")] = np.clip(sd, lo + CLAMP * (hi - lo), lo + (1 - CLAMP) * (hi - lo))
        elif l.type == "binomial":
            n = res["leaf"][j]
            T = n.shape[-1] - 1
            out[(j, "probs")] = (n * np.arange(T + 1)).sum(-1) / (T * n.sum(-1))
    return out


def _evidence(plan, B, seed, missing_fraction=1.0 / 3.0):
    rng = np.random.default_rng(seed)
    gauss = any(l.type == "gaussian" for l in plan.layers)
    x = _random_x(plan, B, rng) * (0.5 if gauss else 1)  # (standard deviations inside the scaled sigmoid's (1e-5, 1))
    miss = rng.random(x.shape) < missing_fraction
    miss[miss.all(axis=1), 0] = False
    return x, miss, np.where(miss, np.nan if gauss else -1.0, x)


@pytest.mark.parametrize("name", ["em_bare", "em_softmax", "cfg1_rbt8", "kat_bernoulli_f0o0", "plan_quadgraph_1x4x4_cp",
                                  "quadgraph_6x6_tucker_k4", "gauss_qt2_k4", "binom_qt2_k4", "qg_cp_k3"])
def test_full_step_reproduces_the_closed_form_targets(name):
    plan, tensors = _any(name)
    _, _, xs = _evidence(plan, 64, 41)
    res = statistics_restated(plan, tensors, xs)
    new = em_restated(plan, tensors, res)
    got, want = normalised_parameters(plan, {**tensors, **new}), _direct_targets(plan, res)
    assert sorted(got) == sorted(want)
    for key, w in want.items():
        assert np.isfinite(got[key]).all()
        assert np.abs(got[key] - w).max() <= 1e-12 * (1 + np.abs(w).max()), key


@pytest.mark.parametrize("missing_fraction", [0.0, 1.0 / 3.0])
@pytest.mark.parametrize("name", ["em_bare", "em_softmax"])
def test_five_em_steps_never_lower_the_likelihood(name, missing_fraction):
    plan, tensors = _any(name)
    x, miss, xs = _evidence(plan, 64, 42, missing_fraction)
    lls = [mean_ll(plan, tensors, x, miss)]
    for _ in range(5):
        tensors = {**tensors, **em_restated(plan, tensors, statistics_restated(plan, tensors, xs))}
        lls.append(mean_ll(plan, tensors, x, miss))
    assert np.isfinite(lls).all()
    assert lls[1] > lls[0]  # (random parameters are no fixed point)
    for before, after in zip(lls, lls[1:]):
        assert after >= before - 1e-9, lls


@pytest.mark.parametrize("name", ["em_bare", "cfg1_rbt8", "plan_quadgraph_1x4x4_cp", "gauss_qt2_k4", "binom_qt2_k4"])
def test_half_step_is_the_midpoint(name):
    plan, tensors = _any(name)
    _, _, xs = _evidence(plan, 64, 43)
    res = statistics_restated(plan, tensors, xs)
    old = normalised_parameters(plan, tensors)
    full = normalised_parameters(plan, {**tensors, **em_restated(plan, tensors, res)})
    half = normalised_parameters(plan, {**tensors, **em_restated(plan, tensors, res, step_size=0.5)})
    for key in old:
        if key[1] == "stddev":  # (the VARIANCE is blended)
            mid, got = 0.5 * (old[key] ** 2 + full[key] ** 2), half[key] ** 2
        else:
            mid, got = 0.5 * (old[key] + full[key]), half[key]
        assert np.abs(got - mid).max() <= 1e-12 * (1 + np.abs(mid).max()), key


@pytest.mark.parametrize("name", ["em_bare", "cfg1_rbt8", "plan_quadgraph_1x4x4_cp", "gauss_qt2_k4", "binom_qt2_k4"])
def test_rows_without_statistics_are_returned_unchanged(name):
    plan, tensors = _any(name)
    _, _, xs = _evidence(plan, 16, 44)
    res = statistics_restated(plan, tensors, xs)
    for field in ("edge", "leaf"):
        for j in res[field]:
            res[field][j][0, 0] = 0  # unit 0 of fold 0 of every layer: no flow
    new = em_restated(plan, tensors, res, step_size=0.7)
    for j, l in enumerate(plan.layers):
        for g in l.params.values():
            n = g.nodes[0].config["tensor"]
            assert np.array_equal(new[n][0, 0], np.asarray(tensors[n], dtype=np.float64)[0, 0]), (j, n)
            if new[n].shape[0] * new[n].shape[1] > 1:  # (the other rows moved)
                assert not np.array_equal(new[n], np.asarray(tensors[n], dtype=np.float64)), (j, n)


def _no_edge_flow(plan, tensors) -> dict:
    """Zero statistics for the sum-type layers of a template plan (their raw tensors have the statistics' shape)."""
    edge = {i: np.zeros(np.asarray(tensors[l.params["weight"].nodes[0].config["tensor"]]).shape)
            for i, l in enumerate(plan.layers) if "weight" in l.params and l.params["weight"].ops[-1] != "mixing_weight"}
    return {"edge": edge, "w": {i: np.ones_like(e) for i, e in edge.items()}}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_clamps_keep_the_raw_values_finite(dtype):
    bound = np.log(CLAMP) - np.log1p(-CLAMP)
    plan, tensors = template("gauss_qt2_k4")
    j = next(j for j, l in enumerate(plan.layers) if l.type == "gaussian")
    F, K = plan.layers[j].num_folds, plan.layers[j].num_output_units
    leaf = np.zeros((F, K, 3))
    leaf[..., 0], leaf[..., 1], leaf[..., 2] = 2.0, 1.0, 0.5  # every row saw 0.5: var_hat = 0
    new = em_restated(plan, tensors, {**_no_edge_flow(plan, tensors), "leaf": {j: leaf}}, dtype=dtype)
    sd = new[plan.layers[j].params["stddev"].nodes[0].config["tensor"]]
    assert np.isfinite(sd).all() and np.allclose(sd, bound, rtol=1e-6)
    plan, tensors = template("binom_qt2_k4")
    j = next(j for j, l in enumerate(plan.layers) if l.type == "binomial")
    l = plan.layers[j]
    T = int(l.config["total_count"])
    leaf = np.zeros((l.num_folds, l.num_output_units, T + 1))
    leaf[0::2, :, 0] = 3.0  # p_hat = 0
    leaf[1::2, :, T] = 3.0  # p_hat = 1
    raw = em_restated(plan, tensors, {**_no_edge_flow(plan, tensors), "leaf": {j: leaf}}, dtype=dtype)[l.params["probs"].nodes[0].config["tensor"]]
    assert np.isfinite(raw).all()
    assert np.allclose(raw[0::2], bound, rtol=1e-6) and np.allclose(raw[1::2], -bound, rtol=1e-6)
