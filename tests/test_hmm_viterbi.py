"""Viterbi decoding of a chain, `HipHMM.viterbi` -- the max-product forward and the walk back, cirkit_amd/csrc/ck_hmm_viterbi.hip --
against an fp64 Viterbi in plain torch over `chain_of(plan)`, which enumeration of all paths pins on a fixture.

Rounding may pick another path of (nearly) the same score, so the criterion is not path identity.  For every live row: (a) the
score is within the project's bound for log values, 1e-4 max(1, |want|) (`_check`); (b) so is the fp64 score of the RETURNED path;
(c) every returned state lies in [0, num_states).  How many rows return another path than the reference's is printed."""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_case
from hmm_restatement import log_emissions
from test_hmm import _case, _check, _model
from test_hmm_posteriors import _binomial_chain, _log_weights
from cirkit_amd.hmm import chain_of


def _observed(plan, tensors, x, integrate_vars=()):
    x = torch.as_tensor(np.asarray(x)).clone()
    if len(integrate_vars):
        x[:, list(integrate_vars)] = float("nan") if x.is_floating_point() else -1
    return log_emissions(plan, tensors, x)


def viterbi(plan, tensors, x, integrate_vars=()):
    """((B, T) states by STEP, (B,) score) in fp64: delta = max_i(log W[o, i] + delta[i] + e[i]), backtracked by argmax."""
    e, steps, ws = _observed(plan, tensors, x, integrate_vars), chain_of(plan), _log_weights(plan, tensors)
    delta, back = torch.zeros_like(e[0]), []
    for s, w in zip(steps, ws):
        delta, arg = (w[None] + (delta + e[s.fold])[:, None, :]).max(dim=-1)
        back.append(arg)
    z = [torch.zeros(e.shape[1], dtype=torch.int64)]  # (unit 0 above the last step)
    for arg in reversed(back):
        z.append(arg.gather(1, z[-1][:, None])[:, 0])
    return torch.stack(z[:0:-1], dim=1), delta[:, 0]


def path_score(plan, tensors, x, z, integrate_vars=()):
    """(B,) fp64: sum_s e_s[z_s] + log W_s[z_{s+1} or 0, z_s] of the paths z (B, T) by step."""
    e, steps, ws = _observed(plan, tensors, x, integrate_vars), chain_of(plan), _log_weights(plan, tensors)
    rows = torch.arange(e.shape[1])
    above = [z[:, s + 1] for s in range(len(steps) - 1)] + [torch.zeros_like(z[:, 0])]
    return sum(e[steps[s].fold][rows, z[:, s]] + ws[s][above[s], z[:, s]] for s in range(len(steps)))


def test_reference_matches_enumeration():
    plan, tensors, g = load_case("hmm_cat_t4_k3_shuffled")
    T, K = len(chain_of(plan)), 3
    paths = torch.tensor(list(itertools.product(range(K), repeat=T)))
    scores = torch.stack([path_score(plan, tensors, g["x"], p.expand(len(g["x"]), T)) for p in paths])  # (K^T, B)
    z, score = viterbi(plan, tensors, g["x"])
    assert float((score - scores.max(0).values).abs().max()) <= 1e-12
    assert float((path_score(plan, tensors, g["x"], z) - score).abs().max()) <= 1e-12
    assert torch.equal(z, paths[scores.argmax(0)])


def _check_viterbi(m, plan, tensors, x, states, score, integrate_vars=(), rows=None):
    """Criteria (a) - (c) on `rows` (all of them by default), every one of which must be live."""
    rows = np.arange(len(x)) if rows is None else rows
    var = [s.var for s in chain_of(plan)]
    states, score = states.cpu()[rows], score.cpu()[rows]
    z, want = viterbi(plan, tensors, x[rows], integrate_vars)
    got = states[:, var]
    assert states.dtype == torch.int64 and int(got.min()) >= 0 and int(got.max()) < m.num_states
    print("rows with another path than the reference's:", int((got != z).any(1).sum()), "of", len(rows))
    _check(score, want)
    _check(path_score(plan, tensors, x[rows], got, integrate_vars), want)


@pytest.mark.gpu
@pytest.mark.parametrize("T,K,C,B,shuffled", [
    (1, 3, 3, 1, False), (2, 3, 3, 33, False), (37, 3, 256, 33, True), (1, 32, 3, 33, False), (37, 32, 256, 33, False),
    (2, 64, 3, 1, False), (37, 64, 3, 33, True), (37, 128, 3, 33, False), (2, 160, 256, 33, True), (3, 1024, 3, 33, False)])
def test_viterbi_matches_reference(hip_device, T, K, C, B, shuffled):
    ordering = np.random.default_rng(T + K).permutation(T).tolist() if shuffled else None
    plan, tensors, x = _case(T, K, C, B, ordering=ordering)
    m = _model(plan, tensors, hip_device)
    states, score = m.viterbi(torch.from_numpy(x).to(hip_device))
    assert m.last_launches == 2 and tuple(states.shape) == (B, T)
    _check_viterbi(m, plan, tensors, x, states, score)


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", [(3, 3), (64, 7), (32, 16)])
def test_peaked_parameters(hip_device, K, C):
    plan, tensors, x = _case(37, K, C, 33, scale=30.0)
    m = _model(plan, tensors, hip_device)
    _check_viterbi(m, plan, tensors, x, *m.viterbi(torch.from_numpy(x).to(hip_device)))


@pytest.mark.gpu
def test_missing_entries_zero_mass_and_bad_category(hip_device):
    plan, tensors, x = _case(37, 64, 5, 33)
    m = _model(plan, tensors, hip_device)
    _check_viterbi(m, plan, tensors, x, *m.viterbi(torch.from_numpy(x).to(hip_device), integrate_vars=[0, 5, 36]), [0, 5, 36])
    ragged = x.copy()
    for b in range(33):  # suffixes of different lengths; row 32 loses every entry: the prior's best path
        ragged[b, 37 - min(37, b + 5):] = -1
    _check_viterbi(m, plan, tensors, ragged, *m.viterbi(torch.from_numpy(ragged).to(hip_device)))
    # category 2 of position 3 has no mass in any state: the 7 rows that observe it have no path; row 8 has a category >= C
    tensors["t0"][list(plan.layers[0].scope_idx[:, 0]).index(3), :, 2] = -np.inf
    x[:, 3] = np.arange(33) % 5
    x[8, 20] = 5
    m = _model(plan, tensors, hip_device)
    states, score = m.viterbi(torch.from_numpy(x).to(hip_device))
    dead = x[:, 3] == 2
    assert int(dead.sum()) == 7 and bool(torch.isneginf(score.cpu()[dead]).all()) and bool((states.cpu()[dead] == -1).all())
    assert bool(torch.isnan(score[8])) and bool((states[8] == -1).all())
    _check_viterbi(m, plan, tensors, x, states, score, rows=np.flatnonzero(~dead & (np.arange(33) != 8)))


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
    states, score = (t.clone() for t in m.viterbi(xd))
    assert m.last_launches == 4 + (name == "binomial")
    _check_viterbi(m, plan, tensors, x, states, score)
    for n in (1, 2):
        s, sc = m.viterbi(xd, rows_per_chunk=n)
        assert torch.equal(s, states) and torch.equal(sc, score)
        assert m.last_launches == 4 * -(-len(x) // n) + (name == "binomial")
