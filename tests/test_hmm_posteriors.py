"""Smoothing posteriors of a chain, `HipHMM.state_posteriors` -- the keeping forward and `ck_hmm_backward`, cirkit_amd/csrc/ck_hmm.hip
-- against the fp64 restatement of the FORWARD algorithm alone: gamma is the gradient of log p(x) with respect to the log
emissions, so nothing of the kernel's beta recursion is in the reference.

Bound: |gamma_got - gamma_want| <= 2e-4 absolute -- the project's bound for log values, 1e-4 max(1, |want|) at magnitude <= 1
(everything is relative to the row), once per pass, and |d gamma| <= gamma (1 - gamma) |d log gamma|.  The same recursion in plain
fp32 torch stays at or below 6.7e-5 of the fp64 values on the shapes below (the peaked (32, 16) case; others 1.9e-5)."""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_case
from hmm_restatement import log_emissions
from test_hmm import _case, _check, _model
from cirkit_amd.hmm import chain_of
from cirkit_amd.templates import hmm

BOUND = 2e-4


def _log_weights(plan, tensors):
    names = [plan.layers[s.layer].params["weight"].nodes[0].config["tensor"] for s in chain_of(plan)]
    return [torch.log_softmax(torch.as_tensor(np.asarray(tensors[n]), dtype=torch.float64)[0], dim=-1) for n in names]


def posteriors(plan, tensors, x, integrate_vars=()):
    """((B, D, K), (B,)) fp64: d log p(x_b) / d e_s[b, i] of `hmm_restatement.hmm_log_prob`'s recursion, by variable id."""
    x = torch.as_tensor(np.asarray(x)).clone()
    if len(integrate_vars):
        x[:, list(integrate_vars)] = float("nan") if x.is_floating_point() else -1
    e = log_emissions(plan, tensors, x).requires_grad_()
    steps, v = chain_of(plan), torch.zeros_like(e[0])
    for s, w in zip(steps, _log_weights(plan, tensors)):
        v = torch.logsumexp(w[None] + (v + e[s.fold])[:, None, :], dim=-1)
    (g,) = torch.autograd.grad(v[:, 0].sum(), e)
    out = torch.zeros(e.shape[1], plan.num_variables, e.shape[2], dtype=torch.float64)
    for s in steps:
        out[:, s.var] = g[s.fold]
    return out, v[:, 0].detach()


def _check_gamma(got, want):
    got, want = got.double().cpu(), want.double()
    assert tuple(got.shape) == tuple(want.shape)
    err = float((got - want).abs().max())
    print("largest error / bound:", err / BOUND)
    assert err <= BOUND
    assert float((got.sum(-1) - 1).abs().max()) <= 1e-4


def test_restatement_matches_brute_force():
    plan, tensors, g = load_case("hmm_cat_t4_k3_shuffled")
    steps, ws = chain_of(plan), _log_weights(plan, tensors)
    e = log_emissions(plan, tensors, g["x"])
    T, K = len(steps), e.shape[2]
    want = torch.zeros(e.shape[1], plan.num_variables, K, dtype=torch.float64)
    for z in itertools.product(range(K), repeat=T):  # z[s] the state of step s; the step above it picks the row of W_s
        lp = sum(e[steps[s].fold][:, z[s]] + ws[s][z[s + 1] if s + 1 < T else 0, z[s]] for s in range(T))
        for s in range(T):
            want[:, steps[s].var, z[s]] += lp.exp()
    got, _ = posteriors(plan, tensors, g["x"])
    assert float((got - want / want.sum(-1, keepdim=True)).abs().max()) <= 1e-12


# ---- on the GPU (shapes, seeds and what they cover: tests/test_hmm.py) -------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("T,K,C,B,shuffled", [
    (1, 3, 3, 1, False), (2, 3, 3, 33, False), (37, 3, 256, 33, True), (1, 32, 3, 33, False), (37, 32, 256, 33, False),
    (2, 64, 3, 1, False), (37, 64, 3, 33, True), (37, 128, 3, 33, False), (2, 160, 256, 33, True), (3, 1024, 3, 33, False)])
def test_posteriors_match_restatement(hip_device, T, K, C, B, shuffled):
    ordering = np.random.default_rng(T + K).permutation(T).tolist() if shuffled else None
    plan, tensors, x = _case(T, K, C, B, ordering=ordering)
    m = _model(plan, tensors, hip_device)
    got, lp = m.state_posteriors(torch.from_numpy(x).to(hip_device), return_log_prob=True)
    assert m.last_launches == 2 and tuple(got.shape) == (B, T, K)
    want, want_lp = posteriors(plan, tensors, x)
    _check_gamma(got, want)
    _check(lp, want_lp)


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", [(3, 3), (64, 7), (32, 16)])
def test_peaked_parameters(hip_device, K, C):
    plan, tensors, x = _case(37, K, C, 33, scale=30.0)
    _check_gamma(_model(plan, tensors, hip_device).state_posteriors(torch.from_numpy(x).to(hip_device)), posteriors(plan, tensors, x)[0])


@pytest.mark.gpu
def test_missing_entries_zero_mass_and_bad_category(hip_device):
    plan, tensors, x = _case(37, 64, 5, 33)
    m = _model(plan, tensors, hip_device)
    _check_gamma(m.state_posteriors(torch.from_numpy(x).to(hip_device), integrate_vars=[0, 5, 36]), posteriors(plan, tensors, x, [0, 5, 36])[0])
    ragged = x.copy()
    for b in range(33):  # suffixes of different lengths; row 32 loses every entry: the prior marginal of each state
        ragged[b, 37 - min(37, b + 5):] = -1
    _check_gamma(m.state_posteriors(torch.from_numpy(ragged).to(hip_device)), posteriors(plan, tensors, ragged)[0])
    # category 2 of position 3 has no mass in any state: the 7 rows that observe it are 0 / 0; row 8 has a category >= C
    tensors["t0"][list(plan.layers[0].scope_idx[:, 0]).index(3), :, 2] = -np.inf
    x[:, 3] = np.arange(33) % 5
    x[8, 20] = 5
    got, lp = _model(plan, tensors, hip_device).state_posteriors(torch.from_numpy(x).to(hip_device), return_log_prob=True)
    got, lp = got.cpu(), lp.cpu()
    dead = x[:, 3] == 2
    assert int(dead.sum()) == 7 and bool(torch.isnan(got[dead]).all()) and bool(torch.isneginf(lp[dead]).all())
    assert bool(torch.isnan(got[8]).all()) and bool(torch.isnan(lp[8]))
    keep = ~dead & (np.arange(33) != 8)
    _check_gamma(got[keep], posteriors(plan, tensors, x[keep])[0])


def _binomial_chain():
    rng = np.random.default_rng(3)
    plan = hmm([1, 3, 0, 2], "binomial", 5, input_layer_kwargs={"total_count": 6})
    tensors = {n: rng.standard_normal(s).astype(np.float32) for n, (s, _) in plan.tensors.items()}
    x = rng.integers(0, 7, (9, 4))
    x[2, 1] = -1
    return plan, tensors, x


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hmm_gauss_t3_k4", "binomial"])
def test_other_input_layers_and_chunking(hip_device, name):
    """Per chunk the staging copy, the layer and the two chain launches; one more for the range check of discrete inputs."""
    if name == "binomial":
        plan, tensors, x = _binomial_chain()
    else:
        plan, tensors, g = load_case(name)
        x = g["x"].copy()
        x[1, 2] = float("nan")
    m = _model(plan, tensors, hip_device)
    xd = torch.from_numpy(x).to(hip_device)
    got = m.state_posteriors(xd).clone()
    assert m.last_launches == 4 + (name == "binomial")
    _check_gamma(got, posteriors(plan, tensors, x)[0])
    for n in (1, 2):
        assert torch.equal(m.state_posteriors(xd, rows_per_chunk=n), got)
        assert m.last_launches == 4 * -(-len(x) // n) + (name == "binomial")
