"""Most probable explanation (`HipCircuit.mpe`, cirkit_amd/mpe.py, cirkit_amd/csrc/ck_mpe.hip).

The reference has no max semiring and no MPE query; these tests pin the GPU completion against a numpy fp64 restatement of
the max-product contract (tests/mpe_restatement.py), and against brute force where max-product is exact."""
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_case
from mpe_restatement import mpe_restated

KAT = ["kat_bernoulli_f0o0", "kat_bernoulli_f0o1", "kat_bernoulli_f1o0", "kat_bernoulli_f1o1"]
PLANS = ["kat_bernoulli_f0o0", "kat_bernoulli_f0o1", "kat_bernoulli_f1o0", "kat_bernoulli_f1o1", "kat_gaussian_f1o1",
         "cfg1_rbt8", "binomial_qg6x6_k4", "quadtree_4x4_kron_k3", "plan_quadgraph_1x4x4_cp", "quadgraph_6x6_tucker_k4",
         "pd_gauss_6x6_k4", "cfg2_qt784"]


def _case(name):
    if os.path.exists(os.path.join(GOLDEN, name + "_golden.npz")):
        return load_case(name)[:2]
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.plan import Plan

    plan = Plan.load(os.path.join(GOLDEN, name))
    return plan, init_plan_tensors(plan)


def _deterministic_case(D=6, C=4):
    """categorical -> sum (1 -> 1) -> CP-T (1 unit) over D variables: max-product is the exact MPE."""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import InputSpec, build_plan, fully_factorized

    plan = build_plan(fully_factorized(D), input_layer=InputSpec("categorical", C), num_input_units=1, num_sum_units=1)
    tensors = init_plan_tensors(plan, seed=3)
    return plan, tensors


def _worlds(D, C):
    return np.array(list(itertools.product(range(C), repeat=D)), dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", KAT)
def test_restated_value_is_the_max_over_worlds(name):
    plan, tensors = _case(name)
    w = _worlds(5, 2)
    _, _, lv_all, _ = mpe_restated(plan, tensors, np.zeros((1, 5)), np.ones(5, dtype=bool))
    _, _, lv_w, _ = mpe_restated(plan, tensors, w, np.zeros(5, dtype=bool))
    assert np.isfinite(lv_all[0])
    assert abs(lv_all[0] - lv_w.max()) <= 1e-12 * (1 + abs(lv_all[0]))


@pytest.mark.parametrize("name", KAT + ["cfg1_rbt8", "pd_gauss_6x6_k4", "binomial_qg6x6_k4"])
def test_restated_completion_gives_back_its_value(name):
    plan, tensors = _case(name)
    D, B = plan.num_variables, 64
    rng = np.random.default_rng(1)
    gauss = any(l.type == "gaussian" for l in plan.layers)
    x = rng.normal(size=(B, D)) if gauss else rng.integers(0, 2, size=(B, D)).astype(np.float64)
    mask = rng.random((B, D)) < 0.5
    out, _, lv, _ = mpe_restated(plan, tensors, x, mask)
    assert np.isfinite(out).all() and np.isfinite(lv).all()
    assert (out[~mask] == x[~mask]).all()
    _, _, lv2, _ = mpe_restated(plan, tensors, out, np.zeros(D, dtype=bool))
    assert np.allclose(lv2, lv, rtol=1e-12, atol=1e-12)


def test_restated_completion_is_the_brute_force_argmax_on_a_deterministic_circuit():
    from oracle.torch_oracle import as_torch, evaluate_plan

    from cirkit_amd.sampling import check_plan

    plan, tensors = _deterministic_case()
    check_plan(plan)
    assert [l.type for l in plan.layers] == ["categorical", "sum", "cpt"]
    w = _worlds(6, 4)
    y = evaluate_plan(plan, {k: v.double() for k, v in as_torch(tensors).items()}, torch.from_numpy(w))[:, 0, 0].numpy()
    out, _, lv, _ = mpe_restated(plan, tensors, np.zeros((1, 6)), np.ones(6, dtype=bool))
    assert (out[0] == w[np.argmax(y)]).all()
    assert abs(lv[0] - y.max()) <= 1e-10


def test_mpe_entry_points_are_exported_at_abi_51():
    from cirkit_amd import _capi as capi

    lib = capi.load()
    assert lib.ck_abi_version() == 51
    for n in ("ck_mpe_input_max", "ck_mpe_up_input", "ck_mpe_up_sum", "ck_mpe_up_product", "ck_mpe_walk"):
        assert hasattr(lib, n) and n in capi.SIGNATURES


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


def _check_against_restatement(plan, tensors, x, mask, out, ch, lv, rows=None):
    # The Binomial log-pmf table the device evaluates (ck_param_binomial_table, shared with the forward) is fp32 and off by
    # up to ~1e-4 per entry, which a row sums over its variables: looser bounds there.
    binomial = any(l.type == "binomial" for l in plan.layers)
    rtol, tol = (1e-4, 1e-3) if binomial else (1e-5, 1e-4)
    x_np = x.cpu().numpy().astype(np.float64)
    if rows is not None:
        x_np, mask = x_np[:rows], (mask[:rows] if mask.ndim == 2 and mask.shape[0] > 1 else mask)
        out, ch, lv = out[:rows], [c[:, :rows] for c in ch], lv[:rows]
    out = out.cpu().numpy()
    ch = [c.cpu().numpy() for c in ch]
    lv = lv.cpu().numpy().astype(np.float64)
    ro, chr_, lr, near = mpe_restated(plan, tensors, x_np, mask, tol=tol)
    m = np.broadcast_to(np.asarray(mask).reshape(-1, plan.num_variables), out.shape)
    assert (out[~m] == x.cpu().numpy()[: out.shape[0]][~m]).all()  # observed entries: the evidence, bit for bit
    fin = np.isfinite(lr)
    assert (np.isfinite(lv) == fin).all()
    assert (np.abs(lv[fin] - lr[fin]) <= rtol * np.abs(lr[fin]) + 1e-5).all(), np.abs(lv[fin] - lr[fin]).max()
    disc = _discrete(plan)
    diff = ((out[:, disc] != ro[:, disc]) & ~(np.isnan(out[:, disc]) & np.isnan(ro[:, disc]))).any(axis=1)
    if (~disc).any():
        a, b = out[:, ~disc], ro[:, ~disc]
        diff |= ~((np.abs(a - b) <= 1e-5 * (1 + np.abs(b))) | (np.isnan(a) & np.isnan(b))).all(axis=1)
    for a, b in zip(ch, chr_):
        diff |= (a != b).any(axis=0)
    assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:8]
    assert diff.mean() <= 0.02, diff.mean()


@pytest.mark.gpu
@pytest.mark.parametrize("mask_kind", ["random", "lower_half", "all"])
@pytest.mark.parametrize("name", PLANS)
def test_gpu_mpe_equals_restatement(hip_device, name, mask_kind):
    plan, tensors = _case(name)
    D = plan.num_variables
    N = 256 if name == "cfg2_qt784" else 1024
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(N, seed=77)  # evidence with mass
    if mask_kind == "random":
        mask = np.random.default_rng(5).random((N, D)) < 0.5
    elif mask_kind == "lower_half":
        mask = np.arange(D) >= D // 2
    else:
        mask = np.ones(D, dtype=bool)
    out, ch, lv = hc.mpe(x, torch.from_numpy(mask), return_choices=True, return_log_value=True)
    torch.cuda.synchronize()
    gauss = not _discrete(plan).all()
    assert out.shape == (N, D) and out.dtype == (torch.float32 if gauss else torch.int64) and out.device.type == "cuda"
    sums = [j for j, l in enumerate(plan.layers) if l.type in ("sum", "cpt", "tucker")]
    assert len(ch) == len(sums)
    for c, j in zip(ch, sums):
        assert c.dtype == torch.int32 and tuple(c.shape) == (plan.layers[j].num_folds, N)
    assert lv.shape == (N,) and lv.dtype == torch.float32
    _check_against_restatement(plan, tensors, x, mask, out, ch, lv)
    # self-consistency: the completion, fully observed, has the same max-product value, and lse >= max
    out2, lv2 = hc.mpe(out, [], return_log_value=True)
    assert torch.equal(out2, out)
    assert torch.allclose(lv2, lv, rtol=1e-5, atol=1e-5)
    y = hc(out)[:, 0, 0]
    assert bool((y >= lv - 1e-5 * lv.abs() - 1e-5).all())


@pytest.mark.gpu
def test_gpu_mpe_is_the_brute_force_argmax_on_a_deterministic_circuit(hip_device):
    plan, tensors = _deterministic_case(6, 4)
    hc = _hc(plan, tensors, hip_device)
    w = torch.from_numpy(_worlds(6, 4)).to(hip_device)
    y = hc(w)[:, 0, 0]
    best = w[int(torch.argmax(y))]
    x = torch.full((3, 6), -1, dtype=torch.int64, device=hip_device)
    out, lv = hc.mpe(x, [], return_log_value=True)
    assert bool((out == best).all())
    assert torch.allclose(lv, y.max().expand(3), rtol=1e-5, atol=1e-5)
    # with evidence on two variables: the argmax over the worlds that agree with it
    x[:, 0], x[:, 3] = torch.tensor([0, 1, 2], device=hip_device), 3
    out = hc.mpe(x, [1, 2, 4, 5])
    for r in range(3):
        keep = (w[:, 0] == x[r, 0]) & (w[:, 3] == 3)
        assert torch.equal(out[r], w[keep][int(torch.argmax(y[keep]))])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2_qt784", "pd_gauss_6x6_k4"])
def test_gpu_mpe_chunking_does_not_change_results(hip_device, name):
    plan, tensors = _case(name)
    D, B = plan.num_variables, 300
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(B, seed=8)
    mask = torch.from_numpy(np.random.default_rng(4).random((B, D)) < 0.5)
    res = [hc.mpe(x, mask, return_choices=True, return_log_value=True, rows_per_chunk=r) for r in (None, 1, 7)]
    for out, ch, lv in res[1:]:
        assert torch.equal(out, res[0][0])
        assert all(torch.equal(a, b) for a, b in zip(ch, res[0][1]))
        assert torch.equal(lv, res[0][2])


@pytest.mark.gpu
def test_gpu_mpe_impossible_evidence(hip_device):
    plan, tensors = _case("cfg1_rbt8")
    D, N = plan.num_variables, 512
    hc = _hc(plan, tensors, hip_device)
    cat = plan.layers[0]
    name = cat.params["probs"].nodes[0].config["tensor"]
    v = np.array(hc.store.export(name), dtype=np.float32)
    f, cc = 3, 1
    v[f] = -np.inf
    v[f, ..., cc] = 0.0  # a point mass in one Categorical fold
    hc.store.set(name, v)
    tensors = dict(tensors)
    tensors[name] = v
    var = int(cat.scope_idx[f, 0])
    x = hc.sample(N, seed=9)
    bad = torch.arange(N, device=hip_device) % 2 == 1
    x[bad, var] = cc + 1  # contradicting evidence in half the rows
    mask = np.zeros((N, D), dtype=bool)
    mask[:, [u for u in range(D) if u != var]] = np.random.default_rng(6).random((N, D - 1)) < 0.6
    out, ch, lv = hc.mpe(x, torch.from_numpy(mask), return_choices=True, return_log_value=True)
    m = torch.from_numpy(mask).to(hip_device)
    assert bool((lv[bad] == -np.inf).all()) and bool(torch.isfinite(lv[~bad]).all())
    assert bool((out[bad][m[bad]] == -1).all())
    assert bool((out[~m] == x[~m]).all())
    assert all(bool((c[:, bad] == -1).all()) for c in ch)
    ok = ~bad
    bad_np = bad.cpu().numpy()
    _check_against_restatement(plan, tensors, x[ok], mask[~bad_np], out[ok], [c[:, ok] for c in ch], lv[ok])


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_gpu_mpe_follows_training_steps(hip_device, fused):
    from cirkit_amd.training import HipTrainer

    plan, tensors, g = load_case("cfg2_qt784")
    xb = torch.from_numpy(g["x"].astype(np.int64)).to(hip_device)
    tr = HipTrainer(plan, tensors, device=hip_device, lr=0.05, fused=None if fused else False)
    assert tr.fused == fused
    mask = torch.from_numpy(np.arange(plan.num_variables) >= 392)
    before, lb = tr.circuit.mpe(xb, mask, return_log_value=True)
    for _ in range(3):
        tr.step(xb)
    after, la = tr.circuit.mpe(xb, mask, return_log_value=True)
    assert not torch.equal(lb, la)
    fresh, lf = _hc(plan, tr.parameters(), hip_device).mpe(xb, mask, return_log_value=True)
    assert torch.equal(after, fresh) and torch.equal(la, lf)


@pytest.mark.gpu
def test_gpu_mpe_config4_default_chunks(hip_device):
    plan, tensors = _case("cfg4_pd784")
    D, B = plan.num_variables, 2048
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(B, seed=12)
    mask = np.random.default_rng(8).random((B, D)) < 0.5
    out, ch, lv = hc.mpe(x, torch.from_numpy(mask), return_choices=True, return_log_value=True)
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all()) and bool(torch.isfinite(lv).all())
    m = torch.from_numpy(mask).to(hip_device)
    assert torch.equal(out[~m], x[~m])
    _check_against_restatement(plan, tensors, x, mask, out, ch, lv, rows=32)


@pytest.mark.gpu
def test_gpu_mpe_refusals(hip_device):
    plan, tensors = _case("cfg5_sos_c_k32")
    hc = _hc(plan, tensors, hip_device)
    with pytest.raises(ValueError, match="lse-sum"):
        hc.mpe(torch.zeros((4, plan.num_variables), dtype=torch.int64, device=hip_device), [0])
    plan, tensors = _case("cfg1_rbt8")
    hc = _hc(plan, tensors, hip_device)
    x = torch.zeros((4, plan.num_variables), dtype=torch.int64, device=hip_device)
    with pytest.raises(ValueError):
        hc.mpe(x, torch.ones((4, plan.num_variables + 1), dtype=torch.bool))
    with pytest.raises(ValueError):
        hc.mpe(x, torch.ones((3, plan.num_variables), dtype=torch.bool))
    with pytest.raises(ValueError):
        hc.mpe(x, [plan.num_variables])
    s = hc._sampler
    assert s._key is None and s._zc is None  # refused before anything was prepared or launched
    name = plan.layers[0].params["probs"].nodes[0].config["tensor"]
    v = np.array(hc.store.export(name), dtype=np.float32)
    v[0, 0, 0] = np.nan  # a NaN input parameter: refused by prepare(), as `sample` refuses it
    hc.store.set(name, v)
    with pytest.raises(ValueError, match="NaN"):
        hc.sample(4, seed=1)
    with pytest.raises(ValueError, match="NaN"):
        hc.mpe(x, [0])


@pytest.mark.gpu
def test_gpu_mpe_out_of_range_evidence_is_reported_and_does_not_stick(hip_device):
    plan, tensors = _case("cfg2_qt784")  # Categorical-256
    D, N = plan.num_variables, 128
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(N, seed=4)
    mask = np.arange(D) >= D // 2
    bad = x.clone()
    bad[5, 10] = 300  # an observed category out of range
    out, lv = hc.mpe(bad, torch.from_numpy(mask), return_log_value=True)
    m = torch.from_numpy(mask).to(hip_device)
    assert torch.equal(out[:, ~m], bad[:, ~m])
    assert bool(torch.isnan(lv[5])) and bool((out[5, m] == -1).all())
    keep = torch.arange(N, device=hip_device) != 5
    assert bool(torch.isfinite(lv[keep]).all())
    with pytest.raises(IndexError):  # reported where hc(x) reports it, and cleared by the check
        hc.check_inputs()
    hc.check_inputs()
    out, ch, lv = hc.mpe(x, torch.from_numpy(mask), return_choices=True, return_log_value=True)
    assert bool(torch.isfinite(lv).all())
    _check_against_restatement(plan, tensors, x, mask, out, ch, lv)
    hc.check_inputs()
