"""Conditional sampling given evidence (`HipCircuit.sample_conditional`, cirkit_amd/sampling.py,
cirkit_amd/csrc/ck_sample_cond.hip).

The reference conditions on one observation by compiling a new circuit (symbolic/functional.py:75-135) and its SamplingQuery
refuses the result; these tests pin the batched GPU draw against a numpy fp64 restatement of the same contract
(tests/conditional_restatement.py) draw for draw, and against the exact conditionals of the known-answer circuits."""
import os

import numpy as np
import pytest
import torch

from conditional_restatement import sample_conditional_restated
from conftest import GOLDEN, load_case
from sampling_restatement import sample_restated

scipy_stats = pytest.importorskip("scipy.stats")

KAT = ["kat_bernoulli_f0o0", "kat_bernoulli_f0o1", "kat_bernoulli_f1o0", "kat_bernoulli_f1o1"]
# (variables observed, their values) of the 5-variable known-answer circuits
EVIDENCE = [((0, 2), (1, 0)), ((4,), (1,)), ((1, 3), (0, 1)), ((0, 1, 2, 3), (1, 1, 0, 1))]


def _case(name):
    if os.path.exists(os.path.join(GOLDEN, name + "_golden.npz")):
        return load_case(name)[:2]
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.plan import Plan

    plan = Plan.load(os.path.join(GOLDEN, name))
    return plan, init_plan_tensors(plan)


def _worlds(name):
    """(the 32 worlds (32, 5), their log values log c(x) from the fixture's outputs)."""
    with np.load(os.path.join(GOLDEN, name + "_golden.npz")) as z:
        return z["x"].astype(np.int64), z["y_f32"].astype(np.float64).reshape(-1)


def _codes(x):
    return np.asarray(x).astype(np.int64) @ (1 << np.arange(5)[::-1])


def _exact_conditional(name, obs, val):
    """(expected probability of each of the 32 codes given the evidence, log c(x_O))."""
    w, y = _worlds(name)
    keep = np.all(w[:, list(obs)] == np.asarray(val), axis=1)
    p = np.zeros(32)
    p[_codes(w[keep])] = np.exp(y[keep])
    return p / p.sum(), float(np.log(np.exp(y[keep]).sum()))


def _chi2_p(counts, expected):
    keep = expected >= 5
    obs = np.append(counts[keep], counts[~keep].sum())
    exp = np.append(expected[keep], expected[~keep].sum())
    if exp[-1] == 0:
        assert obs[-1] == 0, "a world without mass was drawn"
        obs, exp = obs[:-1], exp[:-1]
    exp = exp * obs.sum() / exp.sum()
    return float(scipy_stats.chisquare(obs, exp).pvalue)


def _evidence_batch(N, obs, val):
    x = np.full((N, 5), -1, dtype=np.int64)
    x[:, list(obs)] = val
    mask = np.ones(5, dtype=bool)
    mask[list(obs)] = False
    return x, mask


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", ["cfg1_rbt8", "kat_bernoulli_f0o1", "kat_bernoulli_f1o1"])
def test_restatement_with_everything_sampled_is_sample_restated(name):
    plan, tensors = _case(name)
    N, seed = 2048, 0x5EED_0123_4567
    x = np.zeros((N, plan.num_variables), dtype=np.int64)
    out, ch, near, logev = sample_conditional_restated(plan, tensors, x, np.ones(plan.num_variables, dtype=bool), seed)
    xr, chr_, near_r = sample_restated(plan, tensors, N, seed)
    assert np.isfinite(logev).all()
    same = ~(near | near_r)
    assert same.mean() > 0.99
    assert (out[same] == xr[same]).all()
    assert len(ch) == len(chr_) and all((a[:, same] == b[:, same]).all() for a, b in zip(ch, chr_))


@pytest.mark.parametrize("name", KAT)
def test_restatement_draws_the_exact_conditional(name):
    plan, tensors = _case(name)
    N = 1 << 16
    for obs, val in EVIDENCE:
        x, mask = _evidence_batch(N, obs, val)
        out, ch, _, logev = sample_conditional_restated(plan, tensors, x, mask, seed=97)
        p, lev = _exact_conditional(name, obs, val)
        assert (out[:, list(obs)] == np.asarray(val)).all()
        assert np.allclose(logev, lev, rtol=1e-6, atol=1e-6), (logev[:3], lev)
        counts = np.bincount(_codes(out), minlength=32)
        assert _chi2_p(counts, p * N) >= 1e-6, (obs, val)


def test_restatement_rows_without_mass_draw_nothing():
    plan, tensors = _case("kat_bernoulli_f1o1")
    l = plan.layers[0]  # Bernoulli of one variable, raw probabilities: a point mass at 0
    name = l.params["probs"].nodes[0].config["tensor"]
    tensors = dict(tensors)
    p = np.array(tensors[name], dtype=np.float64)
    p[..., 0], p[..., 1] = 1.0, 0.0
    tensors[name] = p
    var = int(l.scope_idx[0, 0])
    x = np.full((8, 5), -1, dtype=np.int64)
    x[:, var] = np.arange(8) % 2  # odd rows: impossible evidence
    out, ch, _, logev = sample_conditional_restated(plan, tensors, x, np.zeros(5, dtype=bool), seed=1)
    bad = np.arange(8) % 2 == 1
    assert np.isneginf(logev[bad]).all() and np.isfinite(logev[~bad]).all()
    assert (out[bad][:, np.arange(5) != var] == -1).all() and (out[~bad] >= 0).all()
    assert all((c[:, bad] == -1).all() and (c[:, ~bad] >= 0).all() for c in ch)


def test_chunk_rows():
    from cirkit_amd.sampling import chunk_rows

    assert chunk_rows(4096, None, 300_804) == [(0, 4096)]  # config 2: 7139 rows fit 2 GiB
    c4 = chunk_rows(2048, None, 2_784_052)  # config 4: 771 rows per chunk
    assert c4 == [(0, 771), (771, 771), (1542, 506)]
    for B, r in [(4096, 1000), (4096, 4096), (4096, 5000), (1, None), (7, 3)]:
        c = chunk_rows(B, r, 1000)
        assert [r0 for r0, _ in c] == list(np.cumsum([0] + [nb for _, nb in c[:-1]]))
        assert sum(nb for _, nb in c) == B and len({nb for _, nb in c}) <= 2 and all(nb > 0 for _, nb in c)
    with pytest.raises(ValueError):
        chunk_rows(16, 0, 1000)


def test_fold_block_offsets_address_the_arena_layout():
    """`val_off[g] + n Ko + k` reaches unit k of row n of global fold g in an arena laid out as `HipCircuit._bind` lays it
    out: every layer's (F, B, Ko) block at its own (aligned) base."""
    from cirkit_amd.sampling import fold_block_offsets

    folds, units, B = [3, 2, 1, 4], [4, 2, 8, 1], 5
    bases, total = [], 0
    for f, k in zip(folds, units):
        bases.append(total)
        total += -(-f * B * k // 64) * 64
    arena = torch.arange(total, dtype=torch.float32)
    views = [arena[b : b + f * B * k].view(f, B, k) for b, f, k in zip(bases, folds, units)]
    off = fold_block_offsets(bases, folds, units, B)
    assert off.dtype == np.int64 and off.shape == (sum(folds),)
    g = 0
    for v, f_, k_ in zip(views, folds, units):
        for f in range(f_):
            for n in range(B):
                assert torch.equal(arena[off[g] + n * k_ : off[g] + (n + 1) * k_], v[f, n])
            g += 1


# ------------------------------------------------------------------------------------------------------------ GPU
def _hc(plan, tensors, dev, **kw):
    from cirkit_amd.circuit import HipCircuit

    return HipCircuit(plan, tensors, device=dev, **kw)


def _discrete(plan):
    d = np.ones(plan.num_variables, dtype=bool)
    for l in plan.layers:
        if l.type == "gaussian":
            d[l.scope_idx[:, 0]] = False
    return d


def _check_against_restatement(plan, tensors, x, mask, out, ch, logev, seed, rows=None, row_ids=None):
    """The GPU result equals the restatement draw for draw, except at rows with a near-boundary draw (few of them)."""
    x_np = x.cpu().numpy()
    if rows is not None:
        x_np, mask = x_np[:rows], (mask[:rows] if mask.ndim == 2 and mask.shape[0] > 1 else mask)
        out, ch, logev = out[:rows], [c[:, :rows] for c in ch], logev[:rows]
    out = out.cpu().numpy()
    ch = [c.cpu().numpy() for c in ch]
    ro, chr_, near, lr = sample_conditional_restated(plan, tensors, x_np, mask, seed, row_ids=row_ids)
    N = out.shape[0]
    m = np.broadcast_to(np.asarray(mask).reshape(-1, plan.num_variables), out.shape)
    assert (out[~m] == x_np[~m]).all()  # observed entries: the evidence, exactly
    lev = logev.cpu().numpy()
    fin = np.isfinite(lr)
    assert (np.isfinite(lev) == fin).all()
    assert np.allclose(lev[fin], lr[fin], rtol=1e-4, atol=1e-3)
    disc = _discrete(plan)
    diff = ((out[:, disc] != ro[:, disc]) & ~(np.isnan(out[:, disc]) & np.isnan(ro[:, disc]))).any(axis=1)
    for a, b in zip(ch, chr_):
        diff |= (a != b).any(axis=0)
    assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:8]
    draws = sum(l.num_folds for l in plan.layers if l.type not in ("hadamard", "kronecker"))
    assert diff.mean() <= max(1e-3, 2e-5 * draws), (diff.mean(), draws)
    if (~disc).any():
        ok = ~diff
        a, b = out[ok][:, ~disc], ro[ok][:, ~disc]
        assert (np.isnan(a) == np.isnan(b)).all()
        a, b = a[~np.isnan(b)], b[~np.isnan(b)]
        assert (np.abs(a - b) <= 1e-4 * (1 + np.abs(b))).all(), np.abs(a - b).max()
    return N


@pytest.mark.gpu
@pytest.mark.parametrize("mask_kind", ["random", "lower_half", "all"])
@pytest.mark.parametrize("name", ["kat_bernoulli_f0o0", "kat_bernoulli_f0o1", "kat_bernoulli_f1o0", "kat_bernoulli_f1o1",
                                  "kat_gaussian_f1o1", "cfg1_rbt8", "binomial_qg6x6_k4", "quadtree_4x4_kron_k3",
                                  "plan_quadgraph_1x4x4_cp", "quadgraph_6x6_tucker_k4", "pd_gauss_6x6_k4", "cfg2_qt784"])
def test_gpu_conditional_equals_restatement(hip_device, name, mask_kind):
    plan, tensors = _case(name)
    D = plan.num_variables
    N = 512 if name == "cfg2_qt784" else 2048
    seed = 0x1234_5678_9ABC
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(N, seed=77)  # evidence with mass
    if mask_kind == "random":
        mask = np.random.default_rng(5).random((N, D)) < 0.5
    elif mask_kind == "lower_half":
        mask = np.arange(D) >= D // 2
    else:
        mask = np.ones(D, dtype=bool)
    out, ch, logev = hc.sample_conditional(x, torch.from_numpy(mask), seed=seed, return_choices=True,
                                           return_log_evidence=True)
    torch.cuda.synchronize()
    gauss = not _discrete(plan).all()
    assert out.shape == (N, D) and out.dtype == (torch.float32 if gauss else torch.int64) and out.device.type == "cuda"
    sums = [j for j, l in enumerate(plan.layers) if l.type in ("sum", "cpt", "tucker")]
    assert len(ch) == len(sums)
    for c, j in zip(ch, sums):
        assert c.dtype == torch.int32 and tuple(c.shape) == (plan.layers[j].num_folds, N)
    assert logev.shape == (N,) and logev.dtype == torch.float32
    _check_against_restatement(plan, tensors, x, mask, out, ch, logev, seed)
    if mask_kind == "all":  # the same Philox stream as sample()
        s = hc.sample(N, seed=seed)
        agree = (s == out).all(1) if not gauss else torch.isclose(s, out, rtol=1e-4, atol=1e-4).all(1)
        assert agree.float().mean().item() > 0.98


@pytest.mark.gpu
@pytest.mark.parametrize("name", KAT)
def test_gpu_exact_conditional(hip_device, name):
    plan, tensors = _case(name)
    hc = _hc(plan, tensors, hip_device)
    N = 1 << 22
    for obs, val in EVIDENCE[:2]:
        x, mask = _evidence_batch(N, obs, val)
        out, logev = hc.sample_conditional(torch.from_numpy(x).to(hip_device), list(np.nonzero(mask)[0]), seed=13,
                                           return_log_evidence=True)
        p, lev = _exact_conditional(name, obs, val)
        assert (out[:, list(obs)] == torch.tensor(val, device=hip_device)).all()
        assert abs(float(logev[0]) - lev) <= 1e-4 * (1 + abs(lev)) and bool((logev == logev[0]).all())
        got = (out * torch.tensor([16, 8, 4, 2, 1], device=hip_device)).sum(1).cpu().numpy()
        assert _chi2_p(np.bincount(got, minlength=32), p * N) >= 1e-6, (obs, val)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2_qt784", "pd_gauss_6x6_k4"])
def test_gpu_log_evidence_is_the_marginal(hip_device, name):
    plan, tensors = _case(name)
    D = plan.num_variables
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(1024, seed=3)
    mask = torch.from_numpy(np.random.default_rng(2).random((1024, D)) < 0.3).to(hip_device)
    _, logev = hc.sample_conditional(x, mask, seed=1, return_log_evidence=True)
    ref = hc(x, integrate_vars=mask)[:, 0, 0]
    assert torch.allclose(logev, ref, rtol=1e-4, atol=1e-3), (logev - ref).abs().max()
    out, logev = hc.sample_conditional(x, [], seed=1, return_log_evidence=True)  # nothing to draw
    assert torch.equal(out, x)
    assert torch.allclose(logev, hc(x)[:, 0, 0], rtol=1e-4, atol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2_qt784", "pd_gauss_6x6_k4"])
def test_gpu_chunking_does_not_change_results(hip_device, name):
    plan, tensors = _case(name)
    D, B = plan.num_variables, 4096
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(B, seed=8)
    mask = torch.from_numpy(np.random.default_rng(4).random((B, D)) < 0.5)
    res = [hc.sample_conditional(x, mask, seed=21, return_choices=True, rows_per_chunk=r) for r in (None, 1000, B)]
    for out, ch in res[1:]:
        assert torch.equal(out, res[0][0])
        assert all(torch.equal(a, b) for a, b in zip(ch, res[0][1]))


@pytest.mark.gpu
def test_gpu_impossible_evidence_draws_nothing(hip_device):
    plan, tensors = _case("cfg1_rbt8")
    D, N = plan.num_variables, 2048
    hc = _hc(plan, tensors, hip_device)
    xq = torch.randint(0, 2, (64, D), device=hip_device)
    # a point mass in one Categorical fold, pushed through the store: probs = softmax(logits) is one-hot at cc
    cat = plan.layers[0]
    name = cat.params["probs"].nodes[0].config["tensor"]
    v = np.array(hc.store.export(name), dtype=np.float32)
    f, cc = 3, 1
    v[f] = -np.inf
    v[f, ..., cc] = 0.0
    hc.store.set(name, v)
    tensors = dict(tensors)
    tensors[name] = v
    var = int(cat.scope_idx[f, 0])
    x = hc.sample(N, seed=9)
    assert (x[:, var] == cc).all()
    bad = torch.arange(N, device=hip_device) % 2 == 1
    x[bad, var] = cc + 1  # contradicting evidence in half the rows
    mask = np.zeros((N, D), dtype=bool)
    mask[:, [v_ for v_ in range(D) if v_ != var]] = np.random.default_rng(6).random((N, D - 1)) < 0.6
    out, ch, logev = hc.sample_conditional(x, torch.from_numpy(mask), seed=31, return_choices=True,
                                           return_log_evidence=True)
    bad_np, m = bad.cpu().numpy(), torch.from_numpy(mask).to(hip_device)
    assert bool((logev[bad] == -np.inf).all()) and bool(torch.isfinite(logev[~bad]).all())
    assert bool((out[bad][m[bad]] == -1).all())
    assert bool((out[~m] == x[~m]).all())
    assert all(bool((c[:, bad] == -1).all()) for c in ch)
    ok = ~bad
    _check_against_restatement(plan, tensors, x[ok], mask[~bad_np], out[ok], [c[:, ok] for c in ch], logev[ok], 31,
                               row_ids=np.nonzero(~bad_np)[0])
    y = hc(xq)  # the process is healthy: the forward still matches the oracle
    from oracle.torch_oracle import as_torch, evaluate_plan

    yr = evaluate_plan(plan, as_torch(tensors), xq.cpu())
    fin = torch.isfinite(yr)
    assert torch.equal(torch.isfinite(y.cpu()), fin)
    assert torch.allclose(y.cpu()[fin].double(), yr[fin].double(), rtol=1e-4, atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_gpu_conditional_draws_follow_training_steps(hip_device, fused):
    from cirkit_amd.training import HipTrainer

    plan, tensors, g = load_case("cfg2_qt784")
    xb = torch.from_numpy(g["x"].astype(np.int64)).to(hip_device)
    tr = HipTrainer(plan, tensors, device=hip_device, lr=0.05, fused=None if fused else False)
    assert tr.fused == fused
    mask = np.arange(plan.num_variables) >= 392
    before = tr.circuit.sample_conditional(xb, torch.from_numpy(mask), seed=21)
    for _ in range(3):
        tr.step(xb)
    after = tr.circuit.sample_conditional(xb, torch.from_numpy(mask), seed=21)
    assert not torch.equal(before, after)
    fresh = _hc(plan, tr.parameters(), hip_device).sample_conditional(xb, torch.from_numpy(mask), seed=21)
    assert torch.equal(after, fresh)


@pytest.mark.gpu
def test_gpu_conditional_config4_default_chunks(hip_device):
    plan, tensors = _case("cfg4_pd784")
    D, B = plan.num_variables, 2048
    hc = _hc(plan, tensors, hip_device)
    assert hc.arena_bytes(1) * B > (2 << 30)  # (the default chunking makes at least two chunks)
    x = hc.sample(B, seed=12)
    mask = np.random.default_rng(8).random((B, D)) < 0.5
    out, ch, logev = hc.sample_conditional(x, torch.from_numpy(mask), seed=40, return_choices=True,
                                           return_log_evidence=True)
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all()) and bool(torch.isfinite(logev).all())
    m = torch.from_numpy(mask).to(hip_device)
    assert torch.equal(out[~m], x[~m])
    _check_against_restatement(plan, tensors, x, mask, out, ch, logev, 40, rows=64)


@pytest.mark.gpu
def test_gpu_conditional_refusals(hip_device):
    plan, tensors = _case("cfg5_sos_c_k32")
    hc = _hc(plan, tensors, hip_device)
    with pytest.raises(ValueError, match="lse-sum"):
        hc.sample_conditional(torch.zeros((4, plan.num_variables), dtype=torch.int64, device=hip_device), [0])
    plan, tensors = _case("cfg1_rbt8")
    hc = _hc(plan, tensors, hip_device)
    x = torch.zeros((4, plan.num_variables), dtype=torch.int64, device=hip_device)
    with pytest.raises(ValueError):
        hc.sample_conditional(x, torch.ones((4, plan.num_variables + 1), dtype=torch.bool))
    with pytest.raises(ValueError):
        hc.sample_conditional(x, torch.ones((3, plan.num_variables), dtype=torch.bool))
    with pytest.raises(ValueError):
        hc.sample_conditional(x, [plan.num_variables])
    s = hc._sampler
    assert s._key is None and s._zc is None  # refused before anything was prepared or launched


@pytest.mark.gpu
def test_gpu_out_of_range_evidence_is_reported_and_does_not_stick(hip_device):
    plan, tensors = _case("cfg2_qt784")  # Categorical-256
    D, N, seed = plan.num_variables, 256, 0x77
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(N, seed=4)
    mask = np.arange(D) >= D // 2
    bad = x.clone()
    bad[5, 10] = 300  # an observed category out of range
    out = hc.sample_conditional(bad, torch.from_numpy(mask), seed=seed)
    m = torch.from_numpy(mask).to(hip_device)
    assert torch.equal(out[:, ~m], bad[:, ~m])
    with pytest.raises(IndexError):  # reported where hc(x) reports it, and cleared by the check
        hc.check_inputs()
    hc.check_inputs()
    out, ch, logev = hc.sample_conditional(x, torch.from_numpy(mask), seed=seed, return_choices=True,
                                           return_log_evidence=True)
    assert bool(torch.isfinite(logev).all())
    _check_against_restatement(plan, tensors, x, mask, out, ch, logev, seed)
    name = plan.layers[0].params["probs"].nodes[0].config["tensor"]
    hc.store.set(name, np.array(hc.store.export(name)))  # a parameter change: the tables are prepared again
    fresh = _hc(plan, tensors, hip_device)
    assert torch.equal(hc.sample(N, seed=9), fresh.sample(N, seed=9))
    again = hc.sample_conditional(x, torch.from_numpy(mask), seed=seed)
    assert torch.equal(again, fresh.sample_conditional(x, torch.from_numpy(mask), seed=seed))
    hc.check_inputs()
