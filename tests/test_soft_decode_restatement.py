"""The restatement of decoding under soft evidence (tests/soft_decode_restatement.py; DESIGN.md section 11, "Decoding under
soft evidence") pinned on the CPU: its draws against the brute-force posterior over the 32 worlds of the known-answer
circuits, its max-product completion against the brute-force argmax on a deterministic circuit, its own consistency on every
plan of the GPU tests, and the share of rows it flags `near` on exactly the inputs of the GPU parity tests
(tests/test_soft_decode.py), which may leave those rows out of the item-for-item comparison."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conditional_restatement import sample_conditional_restated
from conftest import GOLDEN
from mpe_restatement import mpe_restated
from soft_decode_restatement import completion_value, sample_soft_restated, soft_mpe_restated
from test_mpe import _deterministic_case
from test_mpe import _worlds as _all_worlds
from test_sampling_conditional import KAT, _chi2_p, _codes
from test_soft_evidence import KINDS, PLANS, ROWS, _plan, _soft, evidence, hard_evidence

NEW_ENTRY_POINTS = ("ck_soft_max_leaf", "ck_soft_sample_walk", "ck_soft_mpe_walk", "ck_soft_decode_leaf")
NEAR_CAP = 0.05  # the share of rows a GPU parity test may leave out


# Per plan: (every n-th discrete variable soft, seed of the evidence, Philox seed of `sample_soft`); the other variables are
# hard evidence.  A draw is flagged `near` when its uniform lies within 1e-5 of an interior CDF boundary, so a row is flagged
# with probability about 2e-5 x the interior boundaries of all the draws on its tree: 255 per 256-state variable drawn, 31 / 63
# per sum unit of 32 / 64 entries.  That is a few per cent of the rows of the 256-state plans, and one row of 33 is 3 %: the
# number of drawn variables and the seeds below keep every evidence kind of every plan at or under the cap, which the test
# of the cap asserts.
SEED = 0x50F7_DEC0_DE01
INPUTS = {"kat_bernoulli_f0o0": (3, 5, SEED), "binomial_qg6x6_k4": (2, 4, SEED), "quadtree_4x4_kron_k3": (2, 4, SEED),
          "plan_quadgraph_1x4x4_cp": (2, 4, SEED), "quadgraph_6x6_tucker_k4": (2, 6, SEED + 4), "plan_clt_mixed6_cp": (1, 4, SEED),
          "cat17_k3": (1, 4, SEED), "cat256_k32": (1, 6, SEED + 6), "cat256_k64": (2, 4, SEED + 10), "cfg2_qt784": (8, 4, SEED)}


def parity_inputs(name: str, kind: str):
    """(plan, tensors, soft, log_lik (B, S, C), x (B, D), Philox seed) of the GPU parity test of (plan, evidence kind): 70
    rows on the templated plans, 33 on the others; the variables that are not soft are hard evidence, a third of it missing."""
    plan, tensors = _plan(name)
    every, ev_seed, seed = INPUTS[name]
    B = ROWS[-1] if name.startswith("cat") else ROWS[1]
    soft = _soft(plan, every)
    return plan, tensors, soft, evidence(plan, tensors, soft, B, kind, seed=ev_seed), hard_evidence(plan, B, seed=ev_seed), seed


def _log_worlds(plan, tensors, w, integrate=None):
    from oracle.torch_oracle import as_torch, evaluate_plan

    tt = {k: v.double() for k, v in as_torch(tensors).items()}
    mask = None if integrate is None else torch.from_numpy(np.isin(np.arange(w.shape[1]), integrate))
    return evaluate_plan(plan, tt, torch.from_numpy(w), integrate_mask=mask)[:, 0, 0].numpy()


@pytest.mark.parametrize("kind", ["dense", "onehot", "three"])
@pytest.mark.parametrize("name", KAT)
def test_restated_draws_follow_the_brute_force_posterior(name, kind):
    plan, tensors = _plan(name)
    N = 1 << 16
    w = _all_worlds(5, 2)
    y = _log_worlds(plan, tensors, w)
    soft = [0, 1, 3]  # variable 2 is missing, variable 4 observed
    ll1 = evidence(plan, tensors, soft, 1, kind, seed=31)
    x = np.full((N, 5), np.nan)
    x[:, 4] = 1
    out, _, _, logev = sample_soft_restated(plan, tensors, np.broadcast_to(ll1, (N,) + ll1.shape[1:]), x, soft, seed=97)
    lw = y + sum(ll1[0, s, w[:, v]] for s, v in enumerate(soft))
    lw = np.where(w[:, 4] == 1, lw, -np.inf)
    p = np.zeros(32)
    p[_codes(w)] = np.exp(lw) / np.exp(lw).sum()
    # (the evidence integrates the missing variable by the layer's integral, not by the sum of its stored probabilities)
    li = _log_worlds(plan, tensors, w, integrate=[2]) + sum(ll1[0, s, w[:, v]] for s, v in enumerate(soft))
    logz = float(np.log(np.exp(li[(w[:, 4] == 1) & (w[:, 2] == 0)]).sum()))
    assert (out[:, 4] == 1).all() and (out >= 0).all()
    assert np.abs(logev - logz).max() <= 1e-9 * (1 + abs(logz)), np.abs(logev - logz).max()
    assert _chi2_p(np.bincount(_codes(out), minlength=32), p * N) >= 1e-6


def test_restated_soft_mpe_is_the_brute_force_argmax_on_a_deterministic_circuit():
    plan, tensors = _deterministic_case()
    w = _all_worlds(6, 4)
    y = _log_worlds(plan, tensors, w)
    soft = list(range(6))
    ll = evidence(plan, tensors, soft, 8, "dense", seed=32)
    out, _, lv, _ = soft_mpe_restated(plan, tensors, ll, None, soft)
    for n in range(8):
        tot = y + sum(ll[n, s, w[:, v]] for s, v in enumerate(soft))
        assert (out[n] == w[np.argmax(tot)]).all()
        assert abs(lv[n] - tot.max()) <= 1e-10


@pytest.mark.parametrize("name", PLANS)
def test_restated_completion_gives_back_its_value_and_weight_one_is_the_hard_query(name):
    plan, tensors, soft, ll, x, _ = parity_inputs(name, "dense")
    ll, x = ll[:9], x[:9]
    out, ch, lv, _ = soft_mpe_restated(plan, tensors, ll, x, soft)
    assert np.isfinite(lv).all() and np.isfinite(out).all()
    hard = ~np.isnan(x)
    hard[:, soft] = False
    assert (out[hard] == x[hard]).all()
    again = completion_value(plan, tensors, ll, out, soft)
    assert np.abs(again - lv).max() <= 1e-9 * (1 + np.abs(lv).max()), np.abs(again - lv).max()
    # weight 1 everywhere: `mpe` / `sample_conditional` with the soft variables queried
    zero = np.zeros_like(ll)
    mask = np.zeros(plan.num_variables, dtype=bool)
    mask[soft] = True
    out, ch, lv, _ = soft_mpe_restated(plan, tensors, zero, x, soft)
    ro, rch, rlv, _ = mpe_restated(plan, tensors, x, mask)
    assert np.array_equal(out, ro) and all(np.array_equal(a, b) for a, b in zip(ch, rch))
    assert np.abs(lv - rlv).max() <= 1e-12 * (1 + np.abs(rlv).max())
    out, ch, _, logev = sample_soft_restated(plan, tensors, zero, x, soft, SEED)
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # (the oracle's Binomial takes lgamma of an integer tensor in the default dtype)
    try:
        ro, rch, _, rlev = sample_conditional_restated(plan, tensors, x, mask, SEED)
    finally:
        torch.set_default_dtype(default)
    assert np.array_equal(out, ro, equal_nan=True) and all(np.array_equal(a, b) for a, b in zip(ch, rch))
    # (weight 1 on every state is the sum of the stored fp32 probabilities, the hard query's integral is exactly 1: the two
    #  differ by the rounding of the stored rows, 2^-24 relative per variable)
    assert np.abs(logev - rlev).max() <= 1e-6 * (1 + np.abs(rlev).max())


PARITY_CASES = [(n, k) for n in PLANS for k in KINDS] + [("cfg2_qt784", "dense")]  # (the flagship circuit runs once)
NO_ROW_LEFT_OUT = ("cfg2_qt784",)  # `sample_soft` on the GPU: every row compared, the share of differing rows bounded


@pytest.mark.parametrize("name,kind", PARITY_CASES)
def test_rows_flagged_near_stay_under_the_cap_on_the_inputs_of_the_gpu_tests(name, kind):
    """The GPU parity tests skip the rows the restatement flags; at most 5 % of the rows may be flagged, for both queries.
    cfg2_qt784 (784 variables of 256 states, 32 units) has tens of thousands of interior boundaries on a row's tree, and
    nearly every row holds a flagged draw: its share, printed and asserted to be over the cap here, is why the GPU test leaves
    no row of `sample_soft` out there and bounds the share of differing rows over all of them instead.  `soft_mpe` meets the
    cap there too."""
    plan, tensors, soft, ll, x, seed = parity_inputs(name, kind)
    _, _, _, near_m = soft_mpe_restated(plan, tensors, ll, x, soft)
    _, _, near_s, _ = sample_soft_restated(plan, tensors, ll, x, soft, seed)
    print(f"  near rows: soft_mpe {near_m.mean():.3f}, sample_soft {near_s.mean():.3f}")
    assert near_m.mean() <= NEAR_CAP
    if name in NO_ROW_LEFT_OUT:
        assert near_s.mean() > NEAR_CAP  # (were it under the cap, the GPU test should compare item for item there as well)
    else:
        assert near_s.mean() <= NEAR_CAP


def test_soft_decode_entry_points_are_declared_and_exported_at_abi_51():
    from cirkit_amd import _capi as capi
    from cirkit_amd.circuit import HipCircuit

    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "cirkit_hip.h")).read()
    lib = capi.load()
    assert lib.ck_abi_version() == 51
    for n in NEW_ENTRY_POINTS:
        assert n in capi.SIGNATURES and hasattr(lib, n)
        assert f"int {n}(" in header
    assert callable(HipCircuit.soft_mpe) and callable(HipCircuit.sample_soft)


def test_soft_decode_refusals_raise_their_types_without_a_device():
    from cirkit_amd import soft_decode as sd
    from cirkit_amd.plan import Plan
    from cirkit_amd.templates import image_data

    def call(plan, ll, x=None, soft_vars=None):
        hc = SimpleNamespace(user_plan=plan, layers=[])
        with pytest.raises((ValueError, TypeError, NotImplementedError)) as e:
            sd._state(hc, ll, x, soft_vars)
        assert getattr(hc, "_sampler", None) is None
        return e.value

    ll = torch.zeros((4, 16, 256))
    assert isinstance(call(Plan.load(os.path.join(GOLDEN, "cfg5_sos_c_k32")), ll), ValueError)
    emb = image_data((1, 4, 4), "quad-tree-2", input_layer="embedding", num_input_units=4, num_sum_units=4)
    assert isinstance(call(emb, ll), TypeError)
    mixed, _ = _plan("plan_clt_mixed6_cp")
    assert isinstance(call(mixed, torch.zeros((4, 2, 3)), soft_vars=[0, 1]), NotImplementedError)
    plan, _ = _plan("plan_quadgraph_1x4x4_cp")
    assert isinstance(call(plan, ll[:, :15]), ValueError)
    assert isinstance(call(plan, ll, torch.zeros((3, plan.num_variables), dtype=torch.int64)), ValueError)
    for fn in (sd.soft_mpe, sd.sample_soft):
        with pytest.raises(ValueError):
            fn(SimpleNamespace(user_plan=plan, layers=[]), ll, rows_per_chunk=0)
