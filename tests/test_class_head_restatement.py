"""The class head's contract on the CPU: the fp64 restatement (tests/class_head_restatement.py) against torch's fp64 autograd
of the same loss, against `F.cross_entropy`, and -- through the oracle's autograd -- against the reference's own losses and
gradients on a class-conditional circuit (tests/golden/make_class_fixtures.py); then the host-side validation of
cirkit_amd/classification.py, which touches no device."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from class_head_restatement import class_head, uniform_log_prior
from conftest import GOLDEN, load_case


def _synthetic(B, C, seed, prior=True):
    """Rows of every kind: -inf entries, an all -inf row, a NaN, unlabelled rows, a labelled row with a -inf target, a prior
    with one impossible class (C > 2)."""
    rng = np.random.default_rng(seed)
    l = (rng.uniform(-50.0, 0.0, (B, C)) + rng.choice([-3000.0, -300.0, 0.0], (B, 1))).astype(np.float32)
    y = rng.integers(0, C, B).astype(np.int64)
    y[::7] = -1
    pi = None
    if prior:
        raw = rng.normal(size=C)
        if C > 2:
            raw[1] = -np.inf
        pi = (raw - np.log(np.exp(raw[np.isfinite(raw)]).sum())).astype(np.float32)
    kinds = {}
    if C > 1:
        l[rng.random((B, C)) < 0.1] = -np.inf
    if B >= 8:
        l[3, :] = -np.inf
        kinds["all_inf"] = 3
        l[5, C // 2] = np.nan
        kinds["nan"] = 5
        y[6] = C - 1
        l[6, C - 1] = -np.inf
        kinds["target_inf"] = 6
    return l, y, pi, kinds


def _torch_loss(l, y, pi, w_gen, w_disc, gB, live):
    """The same loss with torch.logsumexp / gather over the rows the contract calls live (fp64 autograd)."""
    lt = torch.from_numpy(l.astype(np.float64)).requires_grad_(True)
    j = lt + torch.from_numpy(pi.astype(np.float64))[None, :]
    rows = torch.from_numpy(np.nonzero(live)[0])
    jl = j[rows]
    yl = torch.from_numpy(y)[rows]
    e = torch.logsumexp(jl, dim=1)
    lab = yl >= 0
    jy = jl.gather(1, yl.clamp(min=0)[:, None])[:, 0]
    gen = torch.where(lab, jy, e)
    disc = torch.where(lab, jy - e, torch.zeros_like(e))
    loss = -(w_gen * gen.sum() + w_disc * disc.sum()) / gB
    loss.backward()
    return float(loss.detach()), lt.grad.numpy(), float(gen.sum().detach()), float(disc.sum().detach())


@pytest.mark.parametrize("B,C", [(1, 1), (9, 2), (33, 3), (70, 10), (40, 65)])
@pytest.mark.parametrize("w", [(1.0, 0.0), (0.0, 1.0), (0.3, 1.0)])
def test_restatement_matches_fp64_autograd(B, C, w):
    l, y, pi, kinds = _synthetic(B, C, seed=B * 100 + C)
    gB = B + 5
    h = class_head(l, y, pi, w[0], w[1], global_batch=gB)
    for k in kinds.values():
        assert h.dead[k] and not h.seed[k].any()
    live = ~h.dead
    assert not h.bad and h.stats[2] == live.sum() and h.stats[5] == h.dead.sum() and h.stats[2] + h.stats[5] == B
    if not live.any():
        return
    loss, grad, gen, disc = _torch_loss(l, y, pi, w[0], w[1], gB, live)
    assert abs(h.loss - loss) <= 1e-12 * max(1.0, abs(loss))
    assert abs(h.stats[0] - gen) <= 1e-12 * max(1.0, abs(gen)) and abs(h.stats[1] - disc) <= 1e-12 * max(1.0, abs(disc))
    assert np.isfinite(h.seed).all()
    assert np.abs(h.seed - grad).max() <= 1e-12 * max(np.abs(grad).max(), 1e-300)
    assert not h.seed[np.isneginf(h.joint)].any()  # exactly zero, never NaN
    # posterior: normalised on rows with a finite evidence, and the prediction is its first maximum
    ok = np.isfinite(h.log_evid)
    assert np.abs(np.exp(h.log_post[ok]).sum(1) - 1.0).max() <= 1e-12
    assert (h.pred[ok] == np.argmax(h.log_post[ok], axis=1)).all() and (h.pred[~ok] == -1).all()
    lab = live & (y >= 0)
    assert h.stats[3] == lab.sum() and h.stats[4] == (h.pred[lab] == y[lab]).sum()


def test_restatement_matches_cross_entropy():
    """Labelled rows only, uniform prior: the discriminative term is torch's cross-entropy, its seed the gradient."""
    rng = np.random.default_rng(3)
    B, C = 37, 10
    l = rng.uniform(-80.0, -20.0, (B, C)).astype(np.float32)
    y = rng.integers(0, C, B).astype(np.int64)
    h = class_head(l, y, None, 0.0, 1.0)
    lt = torch.from_numpy(l.astype(np.float64)).requires_grad_(True)
    ce = F.cross_entropy(lt, torch.from_numpy(y))
    ce.backward()
    assert abs(h.loss - float(ce.detach())) <= 1e-12 * abs(float(ce.detach()))
    assert np.abs(h.seed - lt.grad.numpy()).max() <= 1e-12 * np.abs(lt.grad.numpy()).max()
    assert h.stats[2] == h.stats[3] == B and h.stats[5] == 0


def test_bad_labels_are_flagged_and_dead():
    l = np.zeros((4, 3), dtype=np.float32)
    h = class_head(l, np.array([0, 3, -2, -1]))
    assert h.bad and h.dead.tolist() == [False, True, True, False] and not h.seed[1:3].any()
    assert not class_head(l, np.array([0, 2, -1, -1])).bad


@pytest.mark.parametrize("tag,w", [("d", (0.0, 1.0)), ("g", (1.0, 0.0))])
def test_oracle_autograd_with_restated_head_matches_reference_classifier(tag, w):
    """The reference's own `loss.backward()` of the notebook's discriminative / generative loss on
    plan_quadgraph_1x4x4_cp_nc3: the oracle's output, the restated head's loss and seed, the oracle's autograd from that seed.
    Both sides in fp64 (tests/golden/make_class_fixtures.py says why), the bounds those of
    test_oracle_autograd_matches_reference_gradients_*.  (The notebook's generative loss has no prior in it: the head's
    uniform prior adds the constant log C.)"""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.plan import Plan
    from oracle.torch_oracle import as_torch, evaluate_plan

    plan = Plan.load(os.path.join(GOLDEN, "plan_quadgraph_1x4x4_cp_nc3"))
    tensors = init_plan_tensors(plan, seed=0)
    with np.load(os.path.join(GOLDEN, "quadgraph_1x4x4_cp_nc3_class_grads.npz")) as z:
        g = {k: z[k] for k in z.files}
    x = torch.from_numpy(g["x"].astype(np.int64))
    tt = {k: v.double().requires_grad_(True) for k, v in as_torch(tensors).items()}
    torch.set_default_dtype(torch.float64)
    try:
        out = evaluate_plan(plan, tt, x, grad=True)
    finally:
        torch.set_default_dtype(torch.float32)
    assert out.shape == (24, 1, 3) and out.dtype == torch.float64
    h = class_head(out.detach().numpy()[:, 0, :], g["y"], None, w[0], w[1])
    want = float(g["dis_loss"]) if tag == "d" else float(g["gen_loss"]) - float(uniform_log_prior(3)[0])
    assert abs(h.loss - want) <= 1e-6 * abs(want), (h.loss, want)
    out.backward(torch.from_numpy(h.seed)[:, None, :])
    for k in plan.tensors:
        ref = g[f"g{tag}_{k}"]
        assert np.abs(tt[k].grad.numpy() - ref).max() <= 2e-6 * np.abs(ref).max(), k


# ---- host validation: nothing below reaches a device --------------------------------------------------------------------
def _nc3():
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.plan import Plan

    plan = Plan.load(os.path.join(GOLDEN, "plan_quadgraph_1x4x4_cp_nc3"))
    return plan, init_plan_tensors(plan, seed=0)


@pytest.mark.parametrize("prior", [[0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [-np.inf] * 3, [0.0, np.nan, 0.0]])
def test_bad_priors_are_refused_on_the_host(prior):
    from cirkit_amd.classification import HipClassifier, HipClassifierTrainer

    plan, tensors = _nc3()
    with pytest.raises(ValueError):
        HipClassifier(plan, tensors, device="cuda:0", log_prior=prior)
    with pytest.raises(ValueError):
        HipClassifierTrainer(plan, tensors, device="cuda:0", log_prior=prior)


def test_prior_is_normalised_once_and_keeps_impossible_classes():
    from cirkit_amd.classification import normalise_log_prior

    p = normalise_log_prior([np.log(2.0), -np.inf, np.log(6.0)], 3)
    assert p.dtype == np.float32 and np.isneginf(p[1]) and np.allclose(np.exp(p), [0.25, 0.0, 0.75], atol=1e-7)
    assert normalise_log_prior(None, 3) is None
    assert np.array_equal(normalise_log_prior(p, 3), p) or np.abs(normalise_log_prior(p, 3) - p)[[0, 2]].max() <= 1e-7


def test_labels_are_checked_on_the_host():
    from cirkit_amd.classification import check_labels

    assert check_labels(torch.zeros(5, dtype=torch.int64), 5).shape == (5,)
    for y in (torch.zeros(5, dtype=torch.int32), torch.zeros(5), torch.zeros(4, dtype=torch.int64),
              torch.zeros((5, 1), dtype=torch.int64), [0, 1, 2, 0, 1]):
        with pytest.raises(ValueError):
            check_labels(y, 5)


@pytest.mark.parametrize("w", [(-1.0, 1.0), (1.0, -0.5), (float("nan"), 1.0), (float("inf"), 0.0)])
def test_negative_weights_are_refused(w):
    from cirkit_amd.classification import HipClassifierTrainer

    plan, tensors = _nc3()
    with pytest.raises(ValueError):
        HipClassifierTrainer(plan, tensors, device="cuda:0", generative_weight=w[0], discriminative_weight=w[1])


def test_plans_that_are_not_class_conditional_are_refused():
    from cirkit_amd.classification import HipClassifier, HipClassifierTrainer, num_classes
    from cirkit_amd.plan import IDX_NONE, FoldIndex

    plan, tensors = _nc3()
    assert num_classes(plan) == 3
    assert num_classes(load_case("cfg1_rbt8")[0]) == 1  # (one class is a valid edge)
    sq, sq_tensors, _ = load_case("cfg5_sos_c_k32")  # a squared circuit (complex-lse-sum)
    several = copy.copy(plan)
    many = next(i for i, l in enumerate(plan.layers) if l.num_folds > 1)
    several.output = FoldIndex([many], IDX_NONE)  # every fold of an inner layer as an output
    for p, t in ((sq, sq_tensors), (several, tensors)):
        with pytest.raises(NotImplementedError):
            HipClassifier(p, t, device="cuda:0")
        with pytest.raises(NotImplementedError):
            HipClassifierTrainer(p, t, device="cuda:0")
