"""Posterior path sampling of a chain, `HipHMM.sample_posterior` and `HipHMM.sample` -- the keeping forward and the walk back that
draws, cirkit_amd/csrc/ck_hmm_sample.hip -- against an fp64 restatement of the draw contract ("Sampling
paths") in plain numpy over `chain_of(plan)`, which enumeration of all paths and completions pins on a fixture.

The contract: Philox4x32-10, key the halves of the seed, counter (n, s, 0, 0) with n = row S + j and s the step, ONE call per
(sample, step); u = (x >> 8) 2^-24 of word x0 draws the state from exp(t_s[i]) W_s[z_{s+1}, i], of word x1 the emission of a missing
entry from p(c | z_s); a draw is the smallest index with u Total < CDF_i.  The GPU result must equal the restatement draw for draw
except where a uniform lay within `tol` of an interior end of its interval (`near`), where fp32 may choose the neighbour.

`tol` is measured per case on the CPU, not fixed: ten times the largest difference between a draw's normalised CDF formed in fp32
(the hand-off of the keeping forward and the cumulative sums, `_fp32_hand_off`) and in fp64.  A fixed 5e-5 -- ten times the 5e-6
that LAB_NOTES R7.25 records for the fp32 posteriors -- marks 2 tol K of the pairs per draw, 10 % at K = 1024: no seed keeps that
at or below the 5 % the tests allow.  The measured values lie between 1e-6 (the floor) and 3e-5 (peaked parameters); SEED is one
for which every case marks at most 5 %, found on the CPU from the restatement alone."""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_case
from hmm_restatement import hmm_log_prob, log_emissions
from sampling_restatement import philox4x32_10, uniform
from test_hmm import _case, _check, _model
from test_hmm_posteriors import _log_weights
from test_hmm_viterbi import path_score
from test_sampling_conditional import _chi2_p
from cirkit_amd.hmm import chain_of

TOL_FLOOR, SEED = 1e-6, 22


def _emission_table(plan, tensors):
    """(F, K, C) fp64 p(c | state) of the Categorical input layer."""
    layer = next(l for l in plan.layers if l.inputs is None)
    raw = np.asarray(tensors[layer.params["probs"].nodes[0].config["tensor"]])
    return torch.softmax(torch.as_tensor(raw, dtype=torch.float64), dim=-1).numpy()


def _fp32_hand_off(e, ws, folds):
    """The keeping forward's arithmetic in fp32 on the CPU: t_s relative to the row, p = 2^96 exp(t - max t), y = W p, log y from
    the mantissa and the exponent.  Only to MEASURE what fp32 does to a draw's CDF."""
    f32, l2e = np.float32, np.float32(1.4426950408889634)
    ts, la = [], np.zeros_like(e[0], dtype=f32)
    for f, w in zip(folds, ws):
        ts.append(la + e[f].astype(f32))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            top = np.clip(ts[-1].max(-1, keepdims=True), -3.4e38, 3.4e38)
            mant, ex = np.frexp(np.exp2(ts[-1] * l2e + (f32(96) - top * l2e)) @ np.exp(w).astype(f32).T)
            la = ((np.log2(mant) + (ex - 96).astype(f32)) * f32(0.6931471805599453)).astype(f32)
    return ts


def sample_posterior_restated(plan, tensors, x, S, seed, integrate_vars=(), tol=None):
    """(states (B, S, D), completed (B, S, D), near (B, S)): the contract in fp64.  A row without mass has -1 in every state and
    at every missing entry.  `tol` by default: ten times the largest difference between a draw's normalised CDF in fp32 (the
    kernels' arithmetic on the CPU) and in fp64, measured here for the states and for the emissions, never below TOL_FLOOR."""
    x = np.asarray(x).copy()
    x[:, list(integrate_vars)] = -1
    steps, ws = chain_of(plan), [w.numpy() for w in _log_weights(plan, tensors)]
    e, table = log_emissions(plan, tensors, x).numpy(), _emission_table(plan, tensors)
    B, D = x.shape
    ts, v = [], np.zeros_like(e[0])
    for s, w in zip(steps, ws):  # the forward: t_s = v_{s-1} + e_s
        ts.append(v + e[s.fold])
        a = w[None] + ts[-1][:, None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            top = np.where(np.isfinite(a.max(-1)), a.max(-1), 0.0)
            v = top + np.log(np.exp(a - top[..., None]).sum(-1))
    live = np.isfinite(v[:, 0])
    ts32 = _fp32_hand_off(e, ws, [s.fold for s in steps])
    n = np.arange(B, dtype=np.uint64)[:, None] * np.uint64(S) + np.arange(S, dtype=np.uint64)
    gap, err = np.full((2, B, S), 2.0), np.zeros(2)  # per kind of draw: distance of u to an interior end; fp32 error of the CDF

    def draw(kind, rows, rows32, u, on):
        cdf, cdf32 = np.cumsum(rows, axis=-1), np.cumsum(rows32, axis=-1, dtype=np.float32)
        cdf, cdf32 = cdf / cdf[..., -1:], cdf32 / cdf32[..., -1:]
        i = np.argmax(u[..., None] < cdf, axis=-1)
        at = lambda j: np.take_along_axis(cdf, j[..., None], -1)[..., 0]  # noqa: E731
        lo, hi = np.where(i > 0, at(np.maximum(i - 1, 0)), -1.0), np.where(at(i) < 1.0, at(i), 2.0)
        gap[kind] = np.where(on, np.minimum(gap[kind], np.minimum(np.abs(u - lo), np.abs(u - hi))), gap[kind])
        err[kind] = max(err[kind], np.abs(cdf32 - cdf)[np.broadcast_to(on, i.shape)].max(initial=0.0))
        return i

    states = np.full((B, S, D), -1, dtype=np.int64)
    completed = np.repeat(x[:, None, :], S, axis=1)
    z = np.zeros((B, S), dtype=np.int64)  # (unit 0 above the last step)
    for s in range(len(steps) - 1, -1, -1):
        r = philox4x32_10(n, s, 0, 0, seed & 0xFFFFFFFF, seed >> 32)
        on = np.broadcast_to(live[:, None], z.shape)
        logit = np.where(on[..., None], ts[s][:, None, :] + ws[s][z], 0.0)
        t32 = np.where(on[..., None], ts32[s][:, None, :], np.float32(0))
        q32 = np.exp2((t32 - t32.max(-1, keepdims=True)) * np.float32(1.4426950408889634)) * np.exp(ws[s][z]).astype(np.float32)
        z = draw(0, np.exp(logit - logit.max(-1, keepdims=True)), q32, uniform(r[0]), on)
        miss = (x[:, steps[s].var] < 0)[:, None]
        rows = table[steps[s].fold][z]
        with np.errstate(divide="ignore"):
            c = draw(1, rows, np.exp(np.log(rows).astype(np.float32)), uniform(r[1]), miss & on)
        states[:, :, steps[s].var] = np.where(on, z, -1)
        completed[:, :, steps[s].var] = np.where(miss, np.where(on, c, -1), completed[:, :, steps[s].var])
    tols = np.maximum(10 * err, TOL_FLOOR) if tol is None else np.full(2, tol)
    print("tol (states, emissions):", tols)
    return states, completed, (gap[0] < tols[0]) | (gap[1] < tols[1])


def test_restatement_matches_enumeration():
    """One row of the fixture with two entries missing: 20000 draws of (path, completion) against the exact posterior over the 3^4
    paths times the 5^2 completions; the chi-square criterion of tests/test_sampling_conditional.py."""
    plan, tensors, g = load_case("hmm_cat_t4_k3_shuffled")
    steps, (T, K, C, S) = chain_of(plan), (4, 3, 5, 20000)
    x = g["x"][:1].copy()
    x[0, [steps[1].var, steps[3].var]] = -1
    states, completed, _ = sample_posterior_restated(plan, tensors, x, S, seed=SEED)
    paths = torch.tensor(list(itertools.product(range(K), repeat=T)))  # by step, the first the most significant
    tab = np.log(_emission_table(plan, tensors))
    joint = (path_score(plan, tensors, np.repeat(x, len(paths), 0), paths).numpy()[:, None, None]
             + tab[steps[1].fold][paths[:, 1]][:, :, None] + tab[steps[3].fold][paths[:, 3]][:, None, :])  # (K^T, C, C)
    p = np.exp(joint - joint.max())
    code = states[0][:, [s.var for s in steps]] @ K ** np.arange(T - 1, -1, -1)
    code = (code * C + completed[0][:, steps[1].var]) * C + completed[0][:, steps[3].var]
    assert _chi2_p(np.bincount(code, minlength=p.size), p.reshape(-1) / p.sum() * S) >= 1e-6


def _compare(m, plan, tensors, x, S, got, *, rows=None, integrate_vars=()):
    """Every (row, sample) of `rows` not marked `near` equals the restatement; every one has its states in range and its observed
    entries copied; at most 5 % are marked."""
    rows = np.arange(len(x)) if rows is None else rows
    states, completed, near = (a[rows] for a in sample_posterior_restated(plan, tensors, x, S, SEED, integrate_vars))
    gs, gc = (g.cpu().numpy()[rows] for g in got)
    print("marked near:", int(near.sum()), "of", near.size)
    assert near.mean() <= 0.05
    assert np.array_equal(gs[~near], states[~near]) and np.array_equal(gc[~near], completed[~near])
    var = [s.var for s in chain_of(plan)]
    assert gs.dtype == np.int64 and gs[..., var].min() >= 0 and gs[..., var].max() < m.num_states
    given = np.repeat(np.asarray(x)[rows][:, None, :], S, axis=1)
    given[:, :, list(integrate_vars)] = -1
    assert np.array_equal(gc[given >= 0], given[given >= 0])


def _missing_third(x, seed):
    x[np.random.default_rng(seed).random(x.shape) < 1 / 3] = -1
    return x


# the shapes of test_chain_matches_restatement: every lane-group size (8, 16, 32, 64 lanes) and the chunked K > 256 path
@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("T,K,C,B,shuffled", [
    (1, 3, 3, 1, False), (2, 3, 3, 33, False), (37, 3, 256, 33, True), (1, 32, 3, 33, False), (37, 32, 256, 33, False),
    (2, 64, 3, 1, False), (37, 64, 3, 33, True), (37, 128, 3, 33, False), (2, 160, 256, 33, True), (3, 1024, 3, 33, False)])
def test_samples_match_restatement(hip_device, T, K, C, B, shuffled, S):
    ordering = np.random.default_rng(T + K).permutation(T).tolist() if shuffled else None
    plan, tensors, x = _case(T, K, C, B, ordering=ordering)
    x = _missing_third(x, T + K)
    m = _model(plan, tensors, hip_device)
    states, completed, lp = m.sample_posterior(torch.from_numpy(x).to(hip_device), num_samples=S, seed=SEED, return_log_prob=True)
    assert m.last_launches == 3 and tuple(states.shape) == tuple(completed.shape) == (B, S, T)
    _check(lp, hmm_log_prob(plan, tensors, x))
    _compare(m, plan, tensors, x, S, (states, completed))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 64])
def test_peaked_parameters(hip_device, K):
    plan, tensors, x = _case(37, K, 7, 33, scale=30.0)
    x = _missing_third(x, K)
    m = _model(plan, tensors, hip_device)
    _compare(m, plan, tensors, x, 3, m.sample_posterior(torch.from_numpy(x).to(hip_device), num_samples=3, seed=SEED))


@pytest.mark.gpu
def test_edges(hip_device):
    plan, tensors, x = _case(37, 64, 5, 33)
    x = _missing_third(x, 5)
    # category 2 of position 3 has no mass in any state: the 7 rows that observe it have no path; row 8 has a category >= C
    tensors["t0"][list(plan.layers[0].scope_idx[:, 0]).index(3), :, 2] = -np.inf
    x[:, 3] = np.arange(33) % 5
    x[8, 20] = 5
    m, xd = _model(plan, tensors, hip_device), torch.from_numpy(x).to(hip_device)
    states, completed, lp = (t.clone() for t in m.sample_posterior(xd, num_samples=3, seed=SEED, return_log_prob=True))
    dead = (x[:, 3] == 2) | (np.arange(33) == 8)
    assert bool(torch.isneginf(lp.cpu()[x[:, 3] == 2]).all()) and bool(torch.isnan(lp[8]))
    assert bool((states.cpu()[dead] == -1).all())
    assert np.array_equal(completed.cpu().numpy()[dead], np.repeat(np.where(x < 0, -1, x)[dead][:, None, :], 3, axis=1))
    _compare(m, plan, tensors, np.where(x == 5, 0, x), 3, (states, completed), rows=np.flatnonzero(~dead))
    for n in (1, 2):  # chunks of rows: the same bits (the emission table is built by now: two launches a chunk)
        got = m.sample_posterior(xd, num_samples=3, seed=SEED, rows_per_chunk=n, return_log_prob=True)
        assert torch.equal(got[0], states) and torch.equal(got[1], completed) and m.last_launches == 2 * -(-33 // n)
        assert torch.allclose(got[2], lp, rtol=0, atol=0, equal_nan=True)
    assert all(torch.equal(a, b) for a, b in zip(m.sample_posterior(xd, num_samples=3, seed=SEED), (states, completed)))
    assert not torch.equal(m.sample_posterior(xd, num_samples=3, seed=SEED + 1)[0], states)
    # integrate_vars is the same entries set to -1; sample(N) is one row without evidence
    y = x.copy()
    y[:, [0, 5, 36]] = -1
    want = m.sample_posterior(torch.from_numpy(y).to(hip_device), num_samples=3, seed=SEED)
    assert all(torch.equal(a, b) for a, b in zip(m.sample_posterior(xd, [0, 5, 36], num_samples=3, seed=SEED), want))
    xs, zs = m.sample(50, seed=SEED)
    zw, xw = m.sample_posterior(torch.full((1, 37), -1, device=hip_device), num_samples=50, seed=SEED)
    assert tuple(xs.shape) == (50, 37) and torch.equal(xs, xw[0]) and torch.equal(zs, zw[0]) and int(xs.min()) >= 0
    with pytest.raises(ValueError):
        m.sample_posterior(xd, num_samples=0)
    gauss = _model(*load_case("hmm_gauss_t3_k4")[:2], hip_device)
    for refused in (lambda: gauss.sample_posterior(torch.zeros((1, 3), device=hip_device)), lambda: gauss.sample(4)):
        with pytest.raises(NotImplementedError, match="gaussian"):
            refused()
