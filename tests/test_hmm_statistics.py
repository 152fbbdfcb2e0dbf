"""The Baum-Welch E-step of a chain, `HipHMM.expected_statistics` -- the keeping forward, `ck_hmm_backward_stats`, `ck_hmm_pair_sum`
and `ck_hmm_leaf_sum` (cirkit_amd/csrc/ck_hmm.hip, ck_hmm_stats.hip) -- against fp64 autograd of the FORWARD restatement alone: an
expected transition count is the gradient of sum_b log p(x_b) with respect to the log-weight, an emission count the flow
(tests/test_hmm_posteriors.py: posteriors) contracted with the one-hot of x, or with p(c | k) where the entry is missing.  Nothing
of the kernels' beta recursion or pair product is in the reference.

Bound, per entry, with L live rows: |got - want| <= 2e-4 max(want, L / entries of the matrix) -- the project's 2e-4 for a
probability formed from log values of two passes, relative since |dp| <= p |d log p|, floored at the mean entry of a matrix that sums
to L.  The same statistics from plain fp32 torch autograd reach at most 0.56 of it (the peaked (32, 16) case; 0.20 otherwise).
Measured on the MI355X: at most 0.01 of the bound over this file (LAB_NOTES R7.27)."""
import numpy as np
import pytest
import torch

from conftest import load_case
from hmm_restatement import log_emissions
from test_hmm import _case, _check, _model
from test_hmm_posteriors import _log_weights, posteriors
from cirkit_amd.hmm import chain_of

LAUNCHES = 4  # per chunk: keeping forward, statistics backward, pair sum, leaf sum


def statistics(plan, tensors, x):
    """(per step (Ko, K) expected transition counts, (F, K, C) emission counts, (B,) log p) in fp64 over ALL rows of x."""
    x = np.asarray(x)
    steps, ws = chain_of(plan), [w.requires_grad_() for w in _log_weights(plan, tensors)]
    e = log_emissions(plan, tensors, x)
    v = torch.zeros_like(e[0])
    for s, w in zip(steps, ws):
        v = torch.logsumexp(w[None] + (v + e[s.fold])[:, None, :], dim=-1)
    edges = torch.autograd.grad(v[:, 0].sum(), ws)
    layer = next(l for l in plan.layers if l.inputs is None)
    table = torch.softmax(torch.as_tensor(np.asarray(tensors[layer.params["probs"].nodes[0].config["tensor"]]), dtype=torch.float64), dim=-1)
    gamma, leaf = posteriors(plan, tensors, x)[0], torch.zeros_like(table)
    for s in steps:
        xv = torch.as_tensor(x[:, s.var])
        hot = torch.nn.functional.one_hot(xv.clamp(min=0), table.shape[-1]).double()[:, None, :]
        leaf[s.fold] = torch.einsum("bk,bkc->kc", gamma[:, s.var], torch.where((xv < 0)[:, None, None], table[s.fold][None], hot))
    return edges, leaf, v[:, 0].detach()


def _check_counts(got, want, live):
    got, want = got.double().cpu(), want.double()
    assert tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got).all())
    bound = 2e-4 * want.clamp(min=live / want[0].numel())
    worst = float(((got - want).abs() / bound).max())
    print("largest error / bound:", worst)
    assert worst <= 1.0


def _check_statistics(m, plan, tensors, x, res, live=None, integrate_vars=()):
    """Every field of `res` against the reference on the live rows of x (`live`: a bool mask, default all rows)."""
    x = np.asarray(x).copy()
    x[:, list(integrate_vars)] = -1
    live = np.ones(len(x), dtype=bool) if live is None else live
    edges, leaf, lp = statistics(plan, tensors, x[live])
    n, steps = int(live.sum()), chain_of(plan)
    assert int(res.rows) == n and res.rows.dtype == torch.int64 and res.rows.dim() == 0
    assert sorted(res.edge) == sorted(s.layer for s in steps) and list(res.leaf) == [m.input_layer]
    into = torch.zeros_like(res.unit[m.input_layer])
    for s, want in zip(steps, edges):
        _check_counts(res.edge[s.layer], want[None], n)
        assert torch.allclose(res.unit[s.layer], res.edge[s.layer].sum(-1), rtol=1e-6, atol=0)
        into[s.fold] = res.edge[s.layer].sum(-2)[0]
    assert torch.allclose(res.unit[m.input_layer], into, rtol=1e-6, atol=0)
    _check_counts(res.leaf[m.input_layer], leaf, n)
    _check(res.log_evidence[torch.from_numpy(live).to(res.log_evidence.device)], lp)


# the shapes of tests/test_hmm_posteriors.py; then B = 129 = two row slices of 64 and one ragged row of the pair sum and the leaf
# sum (T = 3, K = 32: 3 jobs a slice), and C = 65: a second category slice of the leaf sum
@pytest.mark.gpu
@pytest.mark.parametrize("T,K,C,B,shuffled", [
    (1, 3, 3, 1, False), (2, 3, 3, 33, False), (37, 3, 256, 33, True), (37, 32, 256, 33, False), (37, 64, 3, 33, True),
    (37, 128, 3, 33, False), (2, 160, 256, 33, True), (3, 1024, 3, 33, False), (3, 32, 3, 129, False), (2, 3, 65, 33, False)])
def test_statistics_match_autograd(hip_device, T, K, C, B, shuffled):
    ordering = np.random.default_rng(T + K).permutation(T).tolist() if shuffled else None
    plan, tensors, x = _case(T, K, C, B, ordering=ordering)
    m = _model(plan, tensors, hip_device)
    res = m.expected_statistics(torch.from_numpy(x).to(hip_device))
    assert m.last_launches == LAUNCHES
    assert tuple(res.edge[chain_of(plan)[-1].layer].shape) == (1, 1, K) and tuple(res.leaf[m.input_layer].shape) == (T, K, C)
    _check_statistics(m, plan, tensors, x, res)


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", [(3, 3), (64, 7), (32, 16)])
def test_peaked_parameters(hip_device, K, C):
    plan, tensors, x = _case(37, K, C, 33, scale=30.0)
    m = _model(plan, tensors, hip_device)
    _check_statistics(m, plan, tensors, x, m.expected_statistics(torch.from_numpy(x).to(hip_device)))


@pytest.mark.gpu
def test_missing_entries_zero_mass_and_bad_category(hip_device):
    plan, tensors, x = _case(37, 64, 5, 33)
    m = _model(plan, tensors, hip_device)
    _check_statistics(m, plan, tensors, x, m.expected_statistics(torch.from_numpy(x).to(hip_device), integrate_vars=[0, 5, 36]),
                      integrate_vars=[0, 5, 36])
    ragged = x.copy()
    for b in range(33):  # suffixes of different lengths; row 32 loses every entry
        ragged[b, 37 - min(37, b + 5):] = -1
    _check_statistics(m, plan, tensors, ragged, m.expected_statistics(torch.from_numpy(ragged).to(hip_device)))
    # category 2 of position 3 has no mass in any state: the 7 rows that observe it are dead; so is row 8, with a category >= C
    tensors["t0"][list(plan.layers[0].scope_idx[:, 0]).index(3), :, 2] = -np.inf
    x[:, 3] = np.arange(33) % 5
    x[8, 20] = 5
    m = _model(plan, tensors, hip_device)
    res = m.expected_statistics(torch.from_numpy(x).to(hip_device))
    live = (x[:, 3] != 2) & (np.arange(33) != 8)
    assert int(res.rows) == 25
    _check_statistics(m, plan, tensors, x, res, live=live)
    lp = m.log_prob(torch.from_numpy(x).to(hip_device))
    assert torch.equal(torch.isnan(res.log_evidence), torch.isnan(lp)) and torch.equal(torch.isneginf(res.log_evidence), torch.isneginf(lp))
    assert bool(torch.isnan(lp[8])) and int(torch.isneginf(lp).sum()) == 7


@pytest.mark.gpu
def test_chunking_and_determinism(hip_device):
    plan, tensors, x = _case(37, 64, 3, 33)
    m = _model(plan, tensors, hip_device)
    xd = torch.from_numpy(x).to(hip_device)
    fields = lambda r: [*r.edge.values(), *r.leaf.values(), *r.unit, r.log_evidence, r.rows]  # noqa: E731
    first = m.expected_statistics(xd)
    assert all(torch.equal(a, b) for a, b in zip(fields(first), fields(m.expected_statistics(xd))))
    for n in (1, 32):
        _check_statistics(m, plan, tensors, x, m.expected_statistics(xd, rows_per_chunk=n))
        assert m.last_launches == LAUNCHES * -(-33 // n)


@pytest.mark.gpu
def test_other_input_layers_are_refused(hip_device):
    plan, tensors, g = load_case("hmm_gauss_t3_k4")
    with pytest.raises(NotImplementedError, match="layer 0"):
        _model(plan, tensors, hip_device).expected_statistics(torch.from_numpy(g["x"]).to(hip_device))


@pytest.mark.gpu
def test_one_baum_welch_step_does_not_lower_the_likelihood(hip_device):
    from cirkit_amd.em import HipEMTrainer

    plan, tensors, x = _case(37, 32, 16, 257)
    xd = torch.from_numpy(x).to(hip_device)
    m = _model(plan, tensors, hip_device)
    before = float(m.log_prob(xd).mean())
    trainer = HipEMTrainer(plan, tensors, device=hip_device)
    trainer.apply(m.expected_statistics(xd))
    after = float(_model(plan, trainer.parameters(), hip_device).log_prob(xd).mean())
    print("mean log-likelihood:", before, "->", after)
    assert after >= before - 1e-4 * max(1.0, abs(before))
