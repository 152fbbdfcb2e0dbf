"""Hidden Markov models: `templates.hmm` against plans compiled by the reference (``pgms.hmm``, fixtures ``hmm_*``), and
`HipHMM.log_prob` -- the whole chain in one launch, cirkit_amd/csrc/ck_hmm.hip -- against the fp64 restatement of the forward
algorithm (tests/hmm_restatement.py), which the fixtures' recorded reference outputs pin."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_case
from hmm_restatement import hmm_log_prob
from test_templates import _assert_same_plan
from cirkit_amd.hmm import chain_of
from cirkit_amd.plan import Plan
from cirkit_amd.templates import InputSpec, hmm, quad_tree_plan

FIXTURES = {
    "hmm_cat_t5_k4_c3": dict(ordering=list(range(5)), input_layer="categorical", num_latent_states=4, input_layer_kwargs={"num_categories": 3}),
    "hmm_cat_t4_k3_shuffled": dict(ordering=[2, 0, 3, 1], input_layer="categorical", num_latent_states=3, input_layer_kwargs={"num_categories": 5}),
    "hmm_gauss_t3_k4": dict(ordering=list(range(3)), input_layer="gaussian", num_latent_states=4),
}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_template_matches_reference_plan_and_restatement_its_output(name):
    plan, tensors, g = load_case(name)
    _assert_same_plan(hmm(**FIXTURES[name]), Plan.load(os.path.join(GOLDEN, name)))
    assert np.abs(hmm_log_prob(plan, tensors, g["x"]).numpy() - g["y_f64"].reshape(-1)).max() <= 1e-10


def test_refusals():
    last = hmm([0], "categorical", 4, input_layer_kwargs={"num_categories": 3}).layers[-1]
    assert (last.type, last.num_input_units, last.num_output_units) == ("sum", 4, 1)  # T = 1: the single sum is K -> 1
    for bad in (dict(ordering=[]), dict(ordering=[0, 2]), dict(ordering=[0, 1], input_layer="poisson"),
                dict(ordering=[0, 1], input_layer_kwargs=[{"num_categories": 3}])):
        with pytest.raises(ValueError):
            hmm(**bad)
    with pytest.raises(NotImplementedError, match="layer 1"):
        chain_of(quad_tree_plan((1, 4, 4), input_layer=InputSpec("categorical", 4), sum_product="cp", num_input_units=2, num_sum_units=2))


# ---- on the GPU -----------------------------------------------------------------------------------------------------------
def _case(T, K, C, B, *, scale=1.0, seed=0, ordering=None):
    """(plan, tensors, x): a categorical chain with logits ``scale * N(0, 1)`` and a uniform batch."""
    rng = np.random.default_rng(seed)
    plan = hmm(list(range(T)) if ordering is None else ordering, "categorical", K, input_layer_kwargs={"num_categories": C})
    tensors = {n: (scale * rng.standard_normal(s)).astype(np.float32) for n, (s, _) in plan.tensors.items()}
    return plan, tensors, rng.integers(0, C, (B, T))


def _check(got, want, factor=1.0):
    """The project's bound for log values (tests/test_squared_marginals.py): |got - want| <= 1e-4 max(1, |want|)."""
    got, want = got.double().cpu(), torch.as_tensor(want).double().cpu()
    finite = torch.isfinite(want)
    assert torch.equal(got[~finite], want[~finite])
    err = (got[finite] - want[finite]).abs() / want[finite].abs().clamp(min=1)
    print("largest error / bound:", float(err.max()) / (factor * 1e-4) if err.numel() else 0.0)
    assert bool((err <= factor * 1e-4).all())


def _model(plan, tensors, dev):
    from cirkit_amd.hmm import HipHMM

    return HipHMM(plan, tensors, device=dev)


# K: 3 is padded to 32; 32 and 64 one and two waves; 128 the first K whose steps outgrow a wave's ring of weight units; 160 waves
# with different numbers of blocks; 1024 the largest (ring of 3 units).  B = 33: a second, ragged row tile.
@pytest.mark.gpu
@pytest.mark.parametrize("T,K,C,B,shuffled", [
    (1, 3, 3, 1, False), (2, 3, 3, 33, False), (37, 3, 256, 33, True), (1, 32, 3, 33, False), (37, 32, 256, 33, False),
    (2, 64, 3, 1, False), (37, 64, 3, 33, True), (37, 128, 3, 33, False), (2, 160, 256, 33, True), (3, 1024, 3, 33, False)])
def test_chain_matches_restatement(hip_device, T, K, C, B, shuffled):
    ordering = np.random.default_rng(T + K).permutation(T).tolist() if shuffled else None
    plan, tensors, x = _case(T, K, C, B, ordering=ordering)
    m = _model(plan, tensors, hip_device)
    _check(m.log_prob(torch.from_numpy(x).to(hip_device)), hmm_log_prob(plan, tensors, x))
    assert m.last_launches == 1
    assert tuple(m(torch.from_numpy(x).to(hip_device)).shape) == (B, 1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", [(3, 3), (64, 7), (32, 16)])
def test_peaked_parameters(hip_device, K, C):
    """Logits scaled by 30: log values down to about -800 over 37 steps, emissions more than 80 nats apart between states -- where
    a linear-space recursion without a running scale ends in 0 / 0.  (The kernel's arithmetic in fp32 on the CPU, denormals flushed:
    0.4 % of the bound.)  C stays small: the kernel reads the Categorical layer's fp32 table log(softmax(logits)), as the reference's
    layer computes it, and an entry below e^-87 is -inf there before the kernel sees it; at C = 256 the logits spread over 170 nats,
    30 % of the table is -inf and one row of 33 then differs from the fp64 value by 14 nats -- in fp64 arithmetic on that table too."""
    plan, tensors, x = _case(37, K, C, 33, scale=30.0)
    want = hmm_log_prob(plan, tensors, x)
    assert float(want.min()) < -300
    _check(_model(plan, tensors, hip_device).log_prob(torch.from_numpy(x).to(hip_device)), want)


@pytest.mark.gpu
def test_missing_entries_zero_mass_and_bad_category(hip_device):
    plan, tensors, x = _case(37, 64, 5, 33)
    m = _model(plan, tensors, hip_device)
    _check(m.log_prob(torch.from_numpy(x).to(hip_device), integrate_vars=[0, 5, 36]), hmm_log_prob(plan, tensors, x, [0, 5, 36]))
    ragged = x.copy()
    for b in range(33):  # suffixes of different lengths; row 32 loses every entry
        ragged[b, 37 - min(37, b + 5):] = -1
    got = m.log_prob(torch.from_numpy(ragged).to(hip_device))
    _check(got, hmm_log_prob(plan, tensors, ragged))
    assert abs(float(got[32])) <= 1e-4  # (normalised parameters: nothing observed, log 1)
    # category 2 of position 3 has no mass in any state: the rows that observe it are -inf, not NaN; a category >= C is NaN
    tensors["t0"][list(plan.layers[0].scope_idx[:, 0]).index(3), :, 2] = -np.inf
    x[:, 3] = np.arange(33) % 5
    x[7, 20] = 5
    got = _model(plan, tensors, hip_device).log_prob(torch.from_numpy(x).to(hip_device)).cpu()
    want = hmm_log_prob(plan, tensors, np.where(x == 5, 0, x))
    assert bool(torch.isneginf(want[x[:, 3] == 2]).all()) and bool(torch.isnan(got[7]))
    keep = np.arange(33) != 7
    _check(got[keep], want[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hmm_gauss_t3_k4", "hmm_cat_t4_k3_shuffled"])
def test_fixtures_chunking_and_identity_with_hipcircuit(hip_device, name):
    """The Gaussian fixture goes through the block of emissions its input layer writes (1 + 2 launches per chunk: the staging copy
    and the layer); `rows_per_chunk` does not change a bit; `HipCircuit` on the same plan agrees within twice the bound."""
    from cirkit_amd.circuit import HipCircuit

    plan, tensors, g = load_case(name)
    x = torch.from_numpy(g["x"]).to(hip_device)
    if name == "hmm_gauss_t3_k4":
        x[1, 2] = float("nan")
    m = _model(plan, tensors, hip_device)
    got = m.log_prob(x).clone()
    gauss = name == "hmm_gauss_t3_k4"
    assert m.last_launches == (3 if gauss else 1)
    _check(got, hmm_log_prob(plan, tensors, x.cpu().numpy()))
    for n in (1, 2):
        assert torch.equal(m.log_prob(x, rows_per_chunk=n), got)
        assert m.last_launches == (3 * -(-6 // n) if gauss else 1)
    _check(got, HipCircuit(plan, tensors, device=hip_device)(x)[:, 0, 0], factor=2.0)
    _check(m.log_prob(x, integrate_vars=[1]), hmm_log_prob(plan, tensors, x.cpu().numpy(), [1]))


@pytest.mark.gpu
def test_binomial_chain(hip_device):
    rng = np.random.default_rng(3)
    plan = hmm([1, 3, 0, 2], "binomial", 5, input_layer_kwargs={"total_count": 6})
    tensors = {n: rng.standard_normal(s).astype(np.float32) for n, (s, _) in plan.tensors.items()}
    x = rng.integers(0, 7, (9, 4))
    x[2, 1] = -1
    m = _model(plan, tensors, hip_device)
    _check(m.log_prob(torch.from_numpy(x).to(hip_device), rows_per_chunk=4), hmm_log_prob(plan, tensors, x))
    assert m.last_launches == 3 * 3 + 1  # per chunk the staging copy, the layer and the chain; one launch for the range check
