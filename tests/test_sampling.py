"""Exact ancestral sampling (`HipCircuit.sample`, cirkit_amd/sampling.py).

The reference's SamplingQuery (cirkit/backend/torch/queries.py:187-275) refuses unnormalised circuits and samples bottom
up; these tests pin the GPU sampler against a numpy restatement of the same contract (tests/sampling_restatement.py) draw
for draw, and against the exact distributions of the reference's known-answer circuits."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_case
from sampling_restatement import philox4x32_10, sample_restated

scipy_stats = pytest.importorskip("scipy.stats")


def _case(name):
    if os.path.exists(os.path.join(GOLDEN, name + "_golden.npz")):
        return load_case(name)[:2]
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.plan import Plan

    plan = Plan.load(os.path.join(GOLDEN, name))
    return plan, init_plan_tensors(plan)


def _worlds(name):
    """(codes of the 32 worlds of a 5-variable binary fixture, their exact probabilities exp(y_f32) / Z)."""
    with np.load(os.path.join(GOLDEN, name + "_golden.npz")) as z:
        x, y = z["x"].astype(np.int64), z["y_f32"].astype(np.float64).reshape(-1)
    p = np.exp(y)
    return x @ (1 << np.arange(x.shape[1])[::-1]), p / p.sum()


def _chi2_p(counts, expected):
    keep = expected >= 5  # (cells with tiny expectations merged into one)
    obs = np.append(counts[keep], counts[~keep].sum())
    exp = np.append(expected[keep], expected[~keep].sum())
    if exp[-1] == 0:
        obs, exp = obs[:-1], exp[:-1]
    exp = exp * obs.sum() / exp.sum()
    return float(scipy_stats.chisquare(obs, exp).pvalue)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_philox_known_answer():
    out = philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_restatement_samples_the_exact_unnormalised_distribution():
    plan, tensors = _case("kat_bernoulli_f1o1")  # Z = 318
    x, choices, _ = sample_restated(plan, tensors, 1 << 18, seed=20241015)
    codes, p = _worlds("kat_bernoulli_f1o1")
    got = x.astype(np.int64) @ (1 << np.arange(5)[::-1])
    counts = np.bincount(got, minlength=32)
    expected = np.zeros(32)
    expected[codes] = p * x.shape[0]
    assert _chi2_p(counts, expected) >= 1e-6
    assert len(choices) == 3 and all((c >= 0).all() for c in choices)  # (a tree: every fold is visited)


def test_check_plan_refusals():
    from cirkit_amd.functional import squared_partition_plan
    from cirkit_amd.plan import Plan
    from cirkit_amd.sampling import check_plan
    from cirkit_amd.templates import image_data

    with pytest.raises(ValueError, match="complex-lse-sum"):  # the semiring before the (Embedding) layers
        check_plan(Plan.load(os.path.join(GOLDEN, "cfg5_sos_c_k32")))
    emb = image_data((1, 4, 4), "quad-tree-2", input_layer="embedding", num_input_units=4, num_sum_units=4)
    assert emb.semiring == "lse-sum"
    with pytest.raises(TypeError, match="TorchEmbeddingLayer"):
        check_plan(emb)
    z = squared_partition_plan(image_data((1, 4, 4), "quad-tree-2", input_layer="categorical", num_input_units=4,
                                          num_sum_units=4))
    assert z.semiring == "lse-sum" and "tensordot" in [l.type for l in z.layers]
    with pytest.raises(TypeError, match="TorchConstantValueLayer"):  # (its first layer)
        check_plan(z)
    td = Plan(z.semiring, 0, [l for l in z.layers if l.type != "constant"], z.output)
    with pytest.raises(TypeError, match="TorchTensorDotLayer"):
        check_plan(td)
    multi = Plan.load(os.path.join(GOLDEN, "cfg1_rbt8"))
    multi.layers[0].scope_idx = np.stack([multi.layers[0].scope_idx[:, 0]] * 2, axis=1)
    with pytest.raises(NotImplementedError):
        check_plan(multi)
    check_plan(Plan.load(os.path.join(GOLDEN, "cfg2_qt784")))


# ------------------------------------------------------------------------------------------------------------ GPU
def _hc(plan, tensors, dev, **kw):
    from cirkit_amd.circuit import HipCircuit

    return HipCircuit(plan, tensors, device=dev, **kw)


def _boundary_mismatch(x, ch, xr, chr_, near, discrete: bool):
    """Samples where the GPU and the restatement differ (discrete values or choices); all must be `near` samples."""
    diff = np.zeros(x.shape[0], dtype=bool)
    if discrete:
        diff |= (x != xr).any(axis=1)
    for a, b in zip(ch, chr_):
        diff |= (a != b).any(axis=0)
    return diff


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kat_bernoulli_f0o0", "kat_bernoulli_f0o1", "kat_bernoulli_f1o0", "kat_bernoulli_f1o1",
                                  "kat_gaussian_f1o1", "cfg1_rbt8", "binomial_qg6x6_k4", "quadtree_4x4_kron_k3",
                                  "plan_quadgraph_1x4x4_cp", "quadgraph_6x6_tucker_k4", "pd_gauss_6x6_k4", "cfg2_qt784"])
def test_gpu_sampler_equals_restatement(hip_device, name):
    plan, tensors = _case(name)
    N, seed = 4096, 0x1234_5678_9ABC
    hc = _hc(plan, tensors, hip_device)
    x, ch = hc.sample(N, seed=seed, return_choices=True)
    torch.cuda.synchronize()
    gauss = any(l.type == "gaussian" for l in plan.layers)
    assert x.shape == (N, plan.num_variables) and x.device.type == "cuda"
    assert x.dtype == (torch.float32 if gauss else torch.int64)
    sums = [j for j, l in enumerate(plan.layers) if l.type in ("sum", "cpt", "tucker")]
    assert len(ch) == len(sums)
    for c, j in zip(ch, sums):
        assert c.dtype == torch.int32 and tuple(c.shape) == (plan.layers[j].num_folds, N)
    xr, chr_, near = sample_restated(plan, tensors, N, seed)
    x = x.cpu().numpy()
    ch = [c.cpu().numpy() for c in ch]
    discrete = ~np.zeros(plan.num_variables, dtype=bool)
    for l in plan.layers:
        if l.type == "gaussian":
            discrete[l.scope_idx[:, 0]] = False
    diff = _boundary_mismatch(x[:, discrete], ch, xr[:, discrete], chr_, near, True)
    # every disagreement is a sample with a draw whose uniform fell within 1e-5 of an interval end (fp32 tables against
    # fp64), and they stay rare: at most 2e-5 per draw of a sample (2351 draws at config 2: 0.7 % of its samples measured;
    # the Binomial layers' fp32 log-pmf table, lgamma(256) ~ 1.1e3 in fp32, moves boundaries by ~1e-4 relative: 0.17 %)
    assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:8]
    draws = sum(l.num_folds for l in plan.layers if l.type not in ("hadamard", "kronecker"))
    assert diff.mean() < max(1e-3, 2e-5 * draws), (diff.mean(), draws)
    ok = ~diff
    if gauss:
        a, b = x[ok][:, ~discrete], xr[ok][:, ~discrete]
        assert (np.abs(a - b) <= 1e-4 * (1 + np.abs(b))).all(), np.abs(a - b).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kat_bernoulli_f0o0", "kat_bernoulli_f0o1", "kat_bernoulli_f1o0", "kat_bernoulli_f1o1"])
def test_gpu_exact_unnormalised_distribution(hip_device, name):
    plan, tensors = _case(name)
    hc = _hc(plan, tensors, hip_device)
    N = 1 << 22
    x = hc.sample(N, seed=7)
    got = (x * torch.tensor([16, 8, 4, 2, 1], device=hip_device)).sum(1).cpu().numpy()
    codes, p = _worlds(name)
    expected = np.zeros(32)
    expected[codes] = p * N
    assert _chi2_p(np.bincount(got, minlength=32), expected) >= 1e-6


@pytest.mark.gpu
def test_gpu_gaussian_marginals(hip_device):
    plan, tensors = _case("kat_gaussian_f1o1")  # Z = 44
    hc = _hc(plan, tensors, hip_device)
    N = 1 << 20
    x = hc.sample(N, seed=11).cpu().numpy().astype(np.float64)
    D = plan.num_variables
    logz = float(hc(torch.zeros((1, D), device=hip_device), integrate_vars=list(range(D))).reshape(-1)[0])
    for d in range(D):
        lo, hi = x[:, d].min() - 1.0, x[:, d].max() + 1.0
        grid = np.linspace(lo, hi, 40001)
        xg = torch.zeros((grid.size, D), dtype=torch.float32)
        xg[:, d] = torch.from_numpy(grid)
        y = hc(xg.to(hip_device), integrate_vars=[v for v in range(D) if v != d]).reshape(-1).double().cpu().numpy()
        dens = np.exp(y - logz)
        edges = np.searchsorted(grid, np.quantile(x[:, d], np.linspace(0, 1, 31)[1:-1]))
        cuts = np.concatenate([[0], edges, [grid.size - 1]])
        trapz = getattr(np, "trapezoid", None) or np.trapz
        mass = np.array([trapz(dens[a:b + 1], grid[a:b + 1]) for a, b in zip(cuts[:-1], cuts[1:])])
        assert abs(mass.sum() - 1.0) < 1e-3
        counts = np.histogram(x[:, d], bins=grid[cuts])[0]
        assert _chi2_p(counts, mass * N) >= 1e-6, d


@pytest.mark.gpu
def test_gpu_sampling_at_scale(hip_device):
    plan, tensors = _case("cfg2_qt784")
    hc = _hc(plan, tensors, hip_device)
    N = 1 << 18
    x, ch = hc.sample(N, seed=3, return_choices=True)
    assert int(x.min()) >= 0 and int(x.max()) < 256
    assert all(int(c.min()) >= 0 for c in ch)  # a tree: every fold is on every sample's induced tree
    D = plan.num_variables
    logz = float(hc(torch.zeros((1, D), dtype=torch.int64, device=hip_device), integrate_vars=list(range(D))).reshape(-1)[0])
    for v in (0, 27, 100, 350, 406, 407, 600, 783):
        xv = torch.zeros((256, D), dtype=torch.int64)
        xv[:, v] = torch.arange(256)
        y = hc(xv.to(hip_device), integrate_vars=[u for u in range(D) if u != v]).reshape(-1).double().cpu().numpy()
        p = np.exp(y - logz)
        assert abs(p.sum() - 1.0) < 1e-3
        counts = torch.bincount(x[:, v], minlength=256).cpu().numpy()
        assert _chi2_p(counts, p / p.sum() * N) >= 1e-6, v


@pytest.mark.gpu
def test_gpu_reproducible_and_fresh(hip_device):
    plan, tensors = _case("cfg1_rbt8")
    hc = _hc(plan, tensors, hip_device)
    a, b, c = hc.sample(2048, seed=5), hc.sample(2048, seed=5), hc.sample(2048, seed=6)
    assert torch.equal(a, b) and not torch.equal(a, c)
    torch.manual_seed(99)
    d = hc.sample(2048)
    torch.manual_seed(99)
    assert torch.equal(d, hc.sample(2048))
    # a point mass pushed into one Categorical fold through the store
    cat = plan.layers[0]
    pn = "logits" if "logits" in cat.params else "probs"
    name = cat.params[pn].nodes[0].config["tensor"]
    v = np.array(hc.store.export(name), dtype=np.float32)
    f, cc = 3, 2
    if pn == "logits" or cat.params[pn].nodes[-1].op == "softmax":
        v[f] = 0.0
        v[f, ..., cc] = 50.0
    else:
        v[f] = 0.0
        v[f, ..., cc] = 1.0
    hc.store.set(name, v)
    x = hc.sample(2048, seed=5)
    var = int(cat.scope_idx[f, 0])
    assert (x[:, var] == cc).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_gpu_samples_follow_training_steps(hip_device, fused):
    from cirkit_amd.training import HipTrainer

    plan, tensors, g = load_case("cfg2_qt784")
    xb = torch.from_numpy(g["x"].astype(np.int64)).to(hip_device)
    tr = HipTrainer(plan, tensors, device=hip_device, lr=0.05, fused=None if fused else False)
    assert tr.fused == fused
    before = tr.circuit.sample(4096, seed=21)
    for _ in range(3):
        tr.step(xb)
    after = tr.circuit.sample(4096, seed=21)
    assert not torch.equal(before, after)
    fresh = _hc(plan, tr.parameters(), hip_device).sample(4096, seed=21)
    assert torch.equal(after, fresh)


@pytest.mark.gpu
def test_gpu_negative_weight_is_refused_without_a_fault(hip_device):
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import image_data

    plan = image_data((1, 4, 4), "quad-tree-2", input_layer="categorical", num_input_units=4, num_sum_units=4,
                      sum_weight_activation="none")
    tensors = {k: np.abs(v) for k, v in init_plan_tensors(plan).items()}
    hc = _hc(plan, tensors, hip_device)
    x = torch.randint(0, 256, (16, plan.num_variables), device=hip_device)
    y0 = hc(x).clone()
    hc.sample(64, seed=1)
    name = plan.layers[-1].params["weight"].nodes[0].config["tensor"]
    w = np.array(hc.store.export(name))
    w.reshape(-1)[0] = -0.5
    hc.store.set(name, w)
    with pytest.raises(ValueError, match="negative"):
        hc.sample(64, seed=1)
    hc.store.set(name, tensors[name])  # the refusal left the circuit as it was: forward and sampling work on
    assert torch.allclose(hc(x), y0)
    assert hc.sample(64, seed=1).shape == (64, plan.num_variables)


@pytest.mark.gpu
def test_gpu_sampling_query_wrapper(hip_device):
    from cirkit_amd.sampling import SamplingQuery

    plan, tensors = _case("cfg1_rbt8")
    hc = _hc(plan, tensors, hip_device)
    s, ch = SamplingQuery(hc)(num_samples=1000, seed=4)
    s2, ch2 = hc.sample(1000, seed=4, return_choices=True)
    assert torch.equal(s, s2) and all(torch.equal(a, b) for a, b in zip(ch, ch2))
