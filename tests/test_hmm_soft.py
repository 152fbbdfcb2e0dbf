"""Soft (likelihood) evidence on a chain, `HipHMM.soft_evidence_log_prob` / `soft_state_posteriors` / `soft_posterior_marginals` /
`soft_viterbi` (cirkit_amd/csrc/ck_hmm_soft.hip around the chain kernels), against fp64 torch: soft emissions
``logsumexp_c(log_lik + log p(c | k))``, `hmm_restatement.log_emissions` for the hard variables, the loop of `hmm_log_prob` over
them; both kinds of posterior by autograd, Viterbi a plain max-product loop over the same emissions.  Bounds: `_check` for log
values, 2e-4 absolute for posteriors (tests/test_hmm_posteriors.py).  As in tests/test_hmm_viterbi.py rounding may pick another
path of nearly the same score: the fp64 score of the RETURNED path is held to the score's bound."""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_case
from hmm_restatement import hmm_log_prob, log_emissions
from test_hmm import _case, _check, _model
from test_hmm_posteriors import _log_weights
from cirkit_amd.hmm import chain_of

LAUNCHES = {"soft_evidence_log_prob": 3, "soft_state_posteriors": 4, "soft_posterior_marginals": 5, "soft_viterbi": 4}


def reference(plan, tensors, ll, x, ids, integrate_vars=()):
    """fp64: log Z (B,), state posteriors (B, D, K) by variable, soft posteriors (B, S, C), Viterbi score (B,) and the (F, B, K)
    emissions it ran on.  `ll`: (B, S, C') fp64."""
    layer = next(l for l in plan.layers if l.inputs is None)
    table = torch.log_softmax(torch.as_tensor(np.asarray(tensors[layer.params["probs"].nodes[0].config["tensor"]]), dtype=torch.float64), -1)
    x = torch.full((len(ll), plan.num_variables), -1) if x is None else torch.as_tensor(np.asarray(x)).clone()
    x[:, list(integrate_vars)] = -1
    ll = ll.clone().requires_grad_(True)
    hard, C = log_emissions(plan, tensors, x[:, :plan.num_variables]), table.shape[-1]
    e = torch.stack([torch.logsumexp(ll[:, ids.index(v), None, :C] + table[f][None], -1) if v in ids else hard[f]
                     for f, v in enumerate(int(v) for v in layer.scope_idx[:, 0])])
    e.retain_grad()
    v, d = torch.zeros_like(e[0]), torch.zeros_like(e[0])
    for s, w in zip(chain_of(plan), _log_weights(plan, tensors)):
        v = torch.logsumexp(w[None] + (v + e[s.fold])[:, None, :], dim=-1)
        d = (w[None] + (d + e[s.fold].detach())[:, None, :]).max(dim=-1).values
    v[:, 0].sum().backward()
    post = torch.zeros(len(ll), plan.num_variables, e.shape[-1], dtype=torch.float64)
    for s in chain_of(plan):
        post[:, s.var] = e.grad[s.fold]
    return v[:, 0].detach(), post, ll.grad[:, :, :C], d[:, 0], e.detach()


def path_score(plan, tensors, e, z):
    """(B,) fp64 score of the paths z (B, D) by variable over the emissions e (F, B, K)."""
    steps, ws, rows = chain_of(plan), _log_weights(plan, tensors), torch.arange(e.shape[1])
    above = [z[:, s.var] for s in steps[1:]] + [torch.zeros_like(z[:, 0])]
    return sum(e[s.fold][rows, z[:, s.var]] + w[a, z[:, s.var]] for s, w, a in zip(steps, ws, above))


def _close(name, got, want, bound=2e-4):
    err = float((got.double().cpu() - want).abs().max())
    print(f"{name}: largest error / bound: {err / bound:.3f}")
    assert err <= bound


def _compare(m, plan, tensors, ll, x, ids, integrate_vars=(), dev=None):
    """All four queries against the reference on live rows; the number of launches of each."""
    kw = {"soft_vars": ids, "integrate_vars": list(integrate_vars) or None}
    xd = None if x is None else torch.from_numpy(x).to(dev)
    lld = ll.float().to(dev)
    logz, post, marg, score, e = reference(plan, tensors, ll.float().double(), x, ids, integrate_vars)
    first = "emission" not in m.tables()
    _check(m.soft_evidence_log_prob(lld, xd, **kw), logz)
    assert m.last_launches == LAUNCHES["soft_evidence_log_prob"] + first
    got, lz = m.soft_state_posteriors(lld, xd, return_log_evidence=True, **kw)
    assert m.last_launches == LAUNCHES["soft_state_posteriors"] and tuple(got.shape) == (len(ll), plan.num_variables, m.num_states)
    _check(lz, logz)
    _close("state posteriors", got, post[:, :, :m.num_states])
    got = m.soft_posterior_marginals(lld, xd, **kw)
    assert m.last_launches == LAUNCHES["soft_posterior_marginals"] and tuple(got.shape) == tuple(marg.shape)
    _close("soft posteriors", got, marg)
    states, sc = m.soft_viterbi(lld, xd, **kw)
    assert m.last_launches == LAUNCHES["soft_viterbi"] and states.dtype == torch.int64
    var = [s.var for s in chain_of(plan)]
    assert int(states[:, var].min()) >= 0 and int(states[:, var].max()) < m.num_states
    _check(sc, score)
    _check(path_score(plan, tensors, e, states.cpu()), score)


# K: 3 is padded to 32; C: 3 is padded to 32, 33 and 65 leave a ragged last block of categories; B = 33 a ragged second row tile;
# K = 160 waves with different numbers of unit blocks; K = 1024 the largest tile.
@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("T,K,C,B,shuffled", [
    (1, 3, 3, 1, False), (2, 3, 33, 33, False), (37, 32, 256, 33, False), (37, 64, 3, 33, True), (2, 160, 65, 33, True),
    (3, 1024, 3, 33, False)])
def test_soft_queries_match_reference(hip_device, T, K, C, B, shuffled, mixed):
    ordering = np.random.default_rng(T + K).permutation(T).tolist() if shuffled else None
    plan, tensors, x = _case(T, K, C, B, ordering=ordering)
    rng = np.random.default_rng(7)
    ids = list(range(0, T, 2)) if mixed else list(range(T))
    ll = torch.from_numpy(2.0 * rng.standard_normal((B, len(ids), C)))
    x[rng.random(x.shape) < 0.3] = -1  # (about half the variables soft, the rest observed, -1 or integrated)
    _compare(_model(plan, tensors, hip_device), plan, tensors, ll, x if mixed else None, ids, [1] if mixed and T > 1 else (),
             hip_device)


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", [(3, 3), (64, 7), (32, 16)])
def test_peaked_parameters(hip_device, K, C):
    """Logits scaled by 30, log_lik = 10 N(0, 1), seed 0 of `_case` and seed 7 of the weights."""
    plan, tensors, _ = _case(37, K, C, 33, scale=30.0)
    ll = torch.from_numpy(10.0 * np.random.default_rng(7).standard_normal((33, 37, C)))
    _compare(_model(plan, tensors, hip_device), plan, tensors, ll, None, list(range(37)), (), hip_device)


@pytest.mark.gpu
def test_one_hot_and_all_zero_weights(hip_device):
    plan, tensors, x = _case(37, 64, 5, 33)
    m, xd = _model(plan, tensors, hip_device), torch.from_numpy(x).to(hip_device)
    ll = torch.full((33, 37, 5), -float("inf"), device=hip_device).scatter_(2, xd[:, :, None], 0.0)
    _check(m.soft_evidence_log_prob(ll), m.log_prob(xd).double().cpu())
    _close("state posteriors", m.soft_state_posteriors(ll), m.state_posteriors(xd).double().cpu())
    _check(m.soft_viterbi(ll)[1], m.viterbi(xd)[1].double().cpu())
    _close("one-hot posteriors", m.soft_posterior_marginals(ll), torch.isfinite(ll).double().cpu())
    _check(m.soft_evidence_log_prob(torch.zeros_like(ll)), torch.zeros(33, dtype=torch.float64))


@pytest.mark.gpu
def test_sets_by_enumeration(hip_device):
    plan, tensors, g = load_case("hmm_cat_t4_k3_shuffled")
    m = _model(plan, tensors, hip_device)
    C = next(l for l in plan.layers if l.inputs is None).config["num_categories"]
    allowed = np.random.default_rng(0).random((5, 4, C)) < 0.6
    allowed[:, :, 0] |= ~allowed.any(-1)
    xs = np.array(list(itertools.product(range(C), repeat=4)))
    p = hmm_log_prob(plan, tensors, xs).exp()
    want = torch.stack([p[torch.from_numpy(a[np.arange(4), xs].all(-1))].sum().log() for a in allowed])
    ll = torch.from_numpy(np.where(allowed, 0.0, -np.inf)).float().to(hip_device)
    _check(m.soft_evidence_log_prob(ll), want)


@pytest.mark.gpu
def test_edges(hip_device):
    plan, tensors, x = _case(5, 64, 5, 33)
    m, xd = _model(plan, tensors, hip_device), torch.from_numpy(x).to(hip_device)
    ids, kw = [0, 2, 3], {"soft_vars": [0, 2, 3]}
    ll = torch.from_numpy(2.0 * np.random.default_rng(1).standard_normal((33, 3, 7))).float().to(hip_device)  # (C' = 7 > C = 5)
    clean = [m.soft_evidence_log_prob(ll, xd, **kw), m.soft_state_posteriors(ll, xd, **kw), m.soft_posterior_marginals(ll, xd, **kw),
             *m.soft_viterbi(ll, xd, **kw)]
    _check(clean[0], reference(plan, tensors, ll.double().cpu(), x, ids)[0])
    wide = ll.clone()
    wide[:, :, 5:] = float("nan")  # (columns past C are never read)
    assert torch.equal(m.soft_evidence_log_prob(wide, xd, **kw), clean[0])
    bad, xb = ll.clone(), xd.clone()
    bad[3, 1, :5] = -float("inf")
    bad[8, 0, 2], bad[20, 2, 4], xb[30, 1] = float("nan"), float("inf"), 5
    for chunk in (None, 1, 32):
        got = [m.soft_evidence_log_prob(bad, xb, rows_per_chunk=chunk, **kw), m.soft_state_posteriors(bad, xb, rows_per_chunk=chunk, **kw),
               m.soft_posterior_marginals(bad, xb, rows_per_chunk=chunk, **kw), *m.soft_viterbi(bad, xb, rows_per_chunk=chunk, **kw)]
        assert float(got[0][3]) == -float("inf") and float(got[4][3]) == -float("inf")
        for r in (3, 8, 20, 30):
            assert bool(torch.isnan(got[1][r]).all()) and bool(torch.isnan(got[2][r]).all()) and bool((got[3][r] == -1).all())
        for r in (8, 20, 30):
            assert bool(torch.isnan(got[0][r])) and bool(torch.isnan(got[4][r]))
        keep = torch.tensor([r not in (3, 8, 20, 30) for r in range(33)], device=hip_device)
        for a, b in zip(got, clean):  # (every other row: the bits of the run without them, chunked or not)
            assert torch.equal(a[keep], b[keep])


@pytest.mark.gpu
def test_refusals(hip_device):
    plan, tensors, _ = _case(5, 3, 5, 4)
    m = _model(plan, tensors, hip_device)
    m.log_prob(torch.zeros((4, 5), dtype=torch.int64, device=hip_device))
    ll = torch.zeros((4, 5, 5), device=hip_device)
    for args, kw in [((ll[0],), {}), ((ll[:, :4],), {}), ((ll[:, :, :4],), {}), ((ll, torch.zeros((3, 5), dtype=torch.int64)), {}),
                     ((ll,), {"rows_per_chunk": 0}), ((ll[:, :1],), {"soft_vars": [0], "integrate_vars": [0]})]:
        for query in LAUNCHES:
            with pytest.raises(ValueError):
                getattr(m, query)(*args, **kw)
    assert m.last_launches == 1
    gplan, gtensors, _ = load_case("hmm_gauss_t3_k4")
    gm = _model(gplan, gtensors, hip_device)
    for query in LAUNCHES:
        with pytest.raises(NotImplementedError, match="gaussian"):
            getattr(gm, query)(torch.zeros((2, 3, 4), device=hip_device))
    assert gm.last_launches == 0
