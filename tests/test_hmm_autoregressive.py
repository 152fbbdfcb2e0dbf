"""The chain-rule decomposition of a chain, `HipHMM.autoregressive_log_probs`, `autoregressive_conditionals` and `coding_tables` --
one walk down the chain, cirkit_amd/csrc/ck_hmm_predict.hip -- against the fp64 restatement of the FORWARD algorithm alone:
position j is `hmm_restatement.hmm_log_prob` with ``order[j + 1:]`` summed out minus the same with ``order[j:]`` summed out, and a
conditional the same difference with ``x[b, order[j]]`` set to each category in turn.  Nothing of the kernel's beta recursion is
in the reference.

Bounds: log-probabilities the project's ``1e-4 max(1, |want|)`` (`test_hmm._check`); conditionals 2e-4 absolute, the bound of
tests/test_hmm_posteriors.py by the same derivation (|dp| <= p |d log p|, the log bound once per pass); rows sum to 1 within 1e-4.
The (37, 32, 256, 33) case spends about ten seconds in its reference: 33 x 37 x 256 fp64 forward passes."""
import numpy as np
import pytest
import torch

from autoregressive_restatement import brute_force, quantise
from conftest import load_case
from hmm_restatement import hmm_log_prob
from test_hmm import _case, _check, _model
from cirkit_amd.hmm import chain_of

BOUND = 2e-4


def restated(plan, tensors, x, integrate_vars=()):
    """((B, T), (B, T, C)) fp64: log p(x_{o_j} | observed prefix) -- 0 where the row misses o_j, NaN behind a prefix without mass
    -- and p(X_{o_j} = c | observed prefix), o the generative order."""
    order = [s.var for s in reversed(chain_of(plan))]
    C = next(l for l in plan.layers if l.inputs is None).config["num_categories"]
    x = np.array(x)
    x[:, list(integrate_vars)] = -1
    B, T = x.shape[0], len(order)
    many = lambda rows: torch.cat([hmm_log_prob(plan, tensors, rows[i:i + 2048]) for i in range(0, len(rows), 2048)])  # noqa: E731
    lp, p = torch.zeros(B, T, dtype=torch.float64), torch.zeros(B, T, C, dtype=torch.float64)
    for j in range(T):
        hidden, own = x.copy(), x.copy()
        hidden[:, order[j:]] = -1
        own[:, order[j + 1:]] = -1
        below = hmm_log_prob(plan, tensors, hidden)
        lp[:, j] = hmm_log_prob(plan, tensors, own) - below
        sweep = np.repeat(hidden, C, axis=0)
        sweep[:, order[j]] = np.tile(np.arange(C), B)
        p[:, j] = (many(sweep).view(B, C) - below[:, None]).exp()
    return lp, p


def test_restatement_matches_brute_force():
    plan, tensors, g = load_case("hmm_cat_t4_k3_shuffled")
    order = [s.var for s in reversed(chain_of(plan))]
    lp, p = restated(plan, tensors, g["x"])
    want_p, want_lp = brute_force(plan, tensors, g["x"], order)
    assert np.abs(p.numpy() - want_p).max() <= 1e-10 and np.abs(lp.numpy() - want_lp).max() <= 1e-10


def _check_p(got, want):
    got, want = got.double().cpu(), want.double()
    assert tuple(got.shape) == tuple(want.shape)
    err = float((got - want).abs().max())
    print("largest error / bound:", err / BOUND)
    assert err <= BOUND
    assert float((got.sum(-1) - 1).abs().max()) <= 1e-4


def _both(m, x, **kw):
    xd = torch.from_numpy(x).to(m.device)
    return m.autoregressive_log_probs(xd, **kw).cpu(), m.autoregressive_conditionals(xd, **kw).cpu()


# K = 3: one padded block of states; C = 3, 33, 256: one padded block of categories, one category past a block, 8 blocks dealt to
# 1 or 4 waves; K = 64 two waves; 160 waves with different numbers of blocks; 1024 the ring of 3 units.  B = 33: a second workgroup
# with one live row.
@pytest.mark.gpu
@pytest.mark.parametrize("T,K,C,B,shuffled", [
    (1, 3, 3, 1, False), (2, 3, 33, 33, False), (37, 32, 256, 33, True), (37, 64, 3, 33, False), (2, 160, 256, 33, True),
    (3, 1024, 3, 33, False)])
def test_matches_restatement(hip_device, T, K, C, B, shuffled):
    ordering = np.random.default_rng(T + K).permutation(T).tolist() if shuffled else None
    plan, tensors, x = _case(T, K, C, B, ordering=ordering)
    m = _model(plan, tensors, hip_device)
    assert m.generative_order == (ordering or list(range(T)))
    xd = torch.from_numpy(x).to(hip_device)
    lp = m.autoregressive_log_probs(xd)
    assert m.last_launches == 1 and tuple(lp.shape) == (B, T)
    p = m.autoregressive_conditionals(xd)
    assert m.last_launches == 2 and tuple(p.shape) == (B, T, C)
    p2, lp2 = m.autoregressive_conditionals(xd, return_log_probs=True)
    assert m.last_launches == 1 and torch.equal(p2, p) and torch.equal(lp2, lp)
    want_lp, want_p = restated(plan, tensors, x)
    _check(lp, want_lp)
    _check_p(p, want_p)
    _check(lp.sum(1), m.log_prob(xd))


def _stored_weights(tensors):
    """The logits whose softmax is what the chain kernels receive: fp32 LINEAR transition probabilities, entries below 2^-126 gone."""
    out = dict(tensors)
    for n in tensors:
        if n != "t0":
            w = torch.softmax(torch.from_numpy(tensors[n]), dim=-1)
            out[n] = torch.log(torch.where(w < 2.0 ** -126, torch.zeros_like(w), w)).numpy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("K,C,seed", [(3, 3, 0), (64, 7, 0), (32, 16, 1)])
def test_peaked_parameters(hip_device, K, C, seed):
    """Logits scaled by 30.  The seeds are chosen on the CPU, by the reference alone: it is finite at every position, and it moves by
    less than a tenth of either bound when the transition weights are rounded to what every chain kernel is given -- linear fp32.
    A single POSITION can hinge on a transition of probability below 2^-126 where `log_prob` of the whole row does not: at seed 0
    of (32, 16) the fp64 reference on the stored weights differs from the one on exact weights by 0.24 at one position (row 6,
    position 6: -6.29 against -8.31), the kernel agrees with the former to the digit, and a later position takes it back."""
    plan, tensors, x = _case(37, K, C, 33, scale=30.0, seed=seed)
    want_lp, want_p = restated(plan, tensors, x)
    assert bool(torch.isfinite(want_lp).all())
    stored_lp, stored_p = restated(plan, _stored_weights(tensors), x)
    assert float(((stored_lp - want_lp).abs() / want_lp.abs().clamp(min=1)).max()) <= 1e-5 and float((stored_p - want_p).abs().max()) <= 2e-5
    lp, p = _both(_model(plan, tensors, hip_device), x)
    _check(lp, want_lp)
    _check_p(p, want_p)


@pytest.mark.gpu
def test_missing_entries_and_dead_ends(hip_device):
    plan, tensors, x = _case(37, 64, 5, 33)
    m = _model(plan, tensors, hip_device)
    ragged = x.copy()
    for b in range(33):  # suffixes of different lengths; row 32 loses every entry: forecasts all the way
        ragged[b, 37 - min(37, b + 5):] = -1
    for rows, integrate in ((x, [0, 5, 36]), (ragged, [])):
        lp, p = _both(m, rows, integrate_vars=integrate or None)
        want_lp, want_p = restated(plan, tensors, rows, integrate)
        _check(lp, want_lp)
        _check_p(p, want_p)
        missing = torch.from_numpy(rows < 0)
        missing[:, integrate] = True
        assert bool((lp[missing] == 0).all()) and bool((want_lp[missing] == 0).all())
    # category 2 of variable 3 has no mass in any state: -inf there, NaN behind it; row 8 has a category >= C at variable 20
    tensors["t0"][list(plan.layers[0].scope_idx[:, 0]).index(3), :, 2] = -np.inf
    x[:, 3] = np.arange(33) % 5
    x[8, 20] = 5
    lp, p = _both(_model(plan, tensors, hip_device), x)
    want_lp, want_p = restated(plan, tensors, np.where(x == 5, 0, x))
    dead = x[:, 3] == 2
    assert int(dead.sum()) == 7 and bool(torch.isneginf(lp[dead, 3]).all()) and bool(torch.isneginf(want_lp[dead, 3]).all())
    assert bool(torch.isnan(lp[dead, 4:]).all()) and bool(torch.isnan(p[dead, 4:]).all()) and bool(torch.isnan(want_lp[dead, 4:]).all())
    assert bool(torch.isnan(lp[8, 20:]).all()) and bool(torch.isnan(p[8, 20:]).all())
    _check(lp[dead, :3], want_lp[dead, :3])
    _check_p(p[dead, :4], want_p[dead, :4])
    _check(lp[8, :20], want_lp[8, :20])
    _check_p(p[8, :20], want_p[8, :20])
    keep = ~dead & (np.arange(33) != 8)
    _check(lp[keep], want_lp[keep])
    _check_p(p[keep], want_p[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("j", [0, 17, 36])
def test_causality(hip_device, j):
    """Entries at order[j:] do not reach the conditionals of positions <= j nor the log-probabilities of positions < j (position
    j's own log-probability is that of x[b, order[j]]: it stays when only order[j + 1:] changes) -- bit for bit."""
    T, C = 37, 7
    ordering = np.random.default_rng(5).permutation(T).tolist()
    plan, tensors, x = _case(T, 64, C, 33, ordering=ordering)
    m = _model(plan, tensors, hip_device)
    lp, p = _both(m, x)
    y = x.copy()
    y[:, ordering[j + 1:]] = (y[:, ordering[j + 1:]] + 1 + np.arange(33)[:, None] % (C - 1)) % C
    lp1, p1 = _both(m, y)
    assert torch.equal(lp1[:, :j + 1], lp[:, :j + 1]) and torch.equal(p1[:, :j + 1], p[:, :j + 1])
    y[:, ordering[j]] = (y[:, ordering[j]] + 1) % C
    lp2, p2 = _both(m, y)
    assert torch.equal(lp2[:, :j], lp[:, :j]) and torch.equal(p2[:, :j + 1], p[:, :j + 1])
    assert not torch.equal(lp2[:, j], lp[:, j])


@pytest.mark.gpu
def test_coding_tables(hip_device):
    plan, tensors, x = _case(5, 3, 33, 33)
    m = _model(plan, tensors, hip_device)
    xd = torch.from_numpy(x).to(hip_device)
    p = m.autoregressive_conditionals(xd).cpu().numpy()
    got = m.coding_tables(xd, precision=16)
    assert m.last_launches == 2 and got.dtype == torch.int32 and tuple(got.shape) == (33, 5, 34)
    want = quantise(p.reshape(-1, 33), np.full(33 * 5, 33), 16).reshape(33, 5, 34)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(m.coding_tables(xd, precision=16, rows_per_chunk=7), got) and m.last_launches == 10
    with pytest.raises(ValueError):
        m.coding_tables(xd, precision=7)


@pytest.mark.gpu
def test_refusals(hip_device):
    plan, tensors, g = load_case("hmm_gauss_t3_k4")
    m = _model(plan, tensors, hip_device)
    x = torch.from_numpy(g["x"]).to(hip_device)
    for query in (m.autoregressive_log_probs, m.autoregressive_conditionals, m.coding_tables):
        with pytest.raises(NotImplementedError, match=f"layer {m.input_layer}"):
            query(x)
    plan, tensors, x = _case(2, 3, 3, 2)
    m = _model(plan, tensors, hip_device)
    for bad in (torch.zeros((2, 3), dtype=torch.int64), torch.zeros((0, 2), dtype=torch.int64)):
        with pytest.raises(ValueError):
            m.autoregressive_conditionals(bad)
